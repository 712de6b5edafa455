// gp_vgicp_batch.hip -- the host side of the VGICP path: the factor and the batch, their tuning, the factor / tile tables, pose staging, the arrival protocol of
// the fused finalize and every C entry point (gp_vgicp_factor_*, gp_vgicp_batch_*, gp_debug_*).  The kernels and their launches are gp_vgicp.hip; what both share is
// gp_vgicp_batch.hpp; the stream plan and the host's 6x6 expansion are gp_vgicp_plan.hpp.
//
// Replaces (reference): the per-factor launch loop of src/gtsam_points/cuda/nonlinear_factor_set_gpu.cpp:64-218 and the host side of
// src/gtsam_points/factors/integrated_vgicp_derivatives{,_linearize,_compute,_inliers}.cu.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "gp_host.hpp"
#include "gp_vgicp_batch.hpp"

using gp::expand_rigid_host;
using gp::kFinalizeParts;
using gp::kFinalizePartsMax;
using gp::kFinalizeSplitTiles;
using gp::kResidentWorkgroups;
using gp::launch_error;
using gp::launch_finalize;
using gp::launch_linearize;
using gp::launch_tiles;
using gp::make_stream_plan;
using gp::partials_ptr;
using gp::PoseSource;

namespace {

constexpr int kPlanMinPoints = 65536;  // single factors below this keep the fixed tiles of a batch (their records then do not depend on how they are batched)

// the extents of the batch's sources, for the far-pose rule (takes_rigid_path): one launch per factor whose source arrays changed, one wait for all of them -- here, where
// a table upload synchronises anyway
int measure_extents(gp_vgicp_batch* b) {
  const int F = (int)b->factors.size();
  std::vector<int> todo;
  for (int i = 0; i < F; i++) {
    gp_vgicp_factor* f = b->factors[i];
    if (f->extent_generation == f->generation) continue;
    if (f->n > 0) todo.push_back(i);
    else f->extent = 0.0, f->extent_generation = f->generation;
  }
  if (todo.empty()) return GP_OK;
  gp::DeviceArray d_ext;
  GP_TRY(d_ext.alloc(sizeof(unsigned) * todo.size()));
  GP_HIP(hipMemsetAsync(d_ext.ptr, 0, sizeof(unsigned) * todo.size(), b->stream));
  for (size_t k = 0; k < todo.size(); k++) {
    const gp_vgicp_factor* f = b->factors[todo[k]];
    GP_TRY(gp::launch_source_extent(b->stream, f->points, 3ll * f->n, d_ext.as<unsigned>() + k));
  }
  std::vector<unsigned> h(todo.size());
  GP_HIP(hipMemcpyAsync(h.data(), d_ext.ptr, sizeof(unsigned) * todo.size(), hipMemcpyDeviceToHost, b->stream));
  GP_HIP(hipStreamSynchronize(b->stream));
  for (size_t k = 0; k < todo.size(); k++) {
    gp_vgicp_factor* f = b->factors[todo[k]];
    float v;
    memcpy(&v, &h[k], sizeof(v));
    f->extent = (double)v;
    f->extent_generation = f->generation;
  }
  return GP_OK;
}

int build_table(gp_vgicp_batch* b) {
  const int F = (int)b->factors.size();
  std::vector<gp::FactorDesc> descs((size_t)F);
  std::vector<gp::TileDesc> tiles;
  b->total_points = 0;
  b->use_grid = true;
  bool offsets32 = true;
  b->any_sv = false;
  {
    // the hashed family reads the maps' private line tables, which a map with a block grid builds only now (gp_voxelmap::ensure_private_table)
    bool all_grid = true;
    for (int i = 0; i < F; i++) {
      if (!b->factors[i]->target->loaded()) return gp::fail(GP_ERROR_NOT_LOADED, "VGICP factor: target voxel map is not loaded on the GPU");
      if (!b->factors[i]->target->has_grid) all_grid = false;
    }
    if (!all_grid || b->tuning.kernel == GP_KERNEL_HASHED)
      for (int i = 0; i < F; i++) GP_TRY(const_cast<gp_voxelmap*>(b->factors[i]->target)->ensure_private_table());  // (a cache of the map, not its state)
  }
  for (int i = 0; i < F; i++) {
    const gp_vgicp_factor* f = b->factors[i];
    if (!f->target->loaded()) return gp::fail(GP_ERROR_NOT_LOADED, "VGICP factor: target voxel map is not loaded on the GPU");
    gp::FactorDesc& d = descs[i];
    d.points = f->points;
    d.covs = f->covs;
    d.normals = f->normals;
    d.map = f->target->view();
    d.n = f->n;
    d.surface_validation = (f->surface_validation && f->normals) ? 1 : 0;
    if (!d.map.gblocks) b->use_grid = false;
    if ((int64_t)d.map.num_voxels * 64 >= (int64_t)1 << 32) offsets32 = false;
    if (d.surface_validation) b->any_sv = true;
    b->total_points += f->n;
  }
  // the family this batch really runs
  int fam = b->tuning.kernel;
  if (fam == GP_KERNEL_STREAM && (!b->use_grid || !offsets32)) fam = GP_KERNEL_LOOKAHEAD;
  if ((fam == GP_KERNEL_LOOKAHEAD || fam == GP_KERNEL_GRID_F64) && !b->use_grid) fam = GP_KERNEL_HASHED;
  b->family = fam;
  // the packed source mirrors (gp::SourceMirror): built once per cloud, here, where a table upload synchronises anyway.  The batch streams them when
  // EVERY factor with a full chunk has a usable one (a cloud with an unsymmetric covariance has none and keeps the whole batch on the caller's arrays)
  b->packed = false;
  if (fam == GP_KERNEL_STREAM && b->tuning.source_mirror) {
    bool all = F > 0;
    for (int i = 0; i < F; i++) {
      gp_vgicp_factor* f = b->factors[i];
      if (!f->mirror_tried) {
        GP_TRY(gp::acquire_source_mirror(f->points, f->covs, f->n, f->device, b->stream, &f->mirror));
        f->mirror_tried = true;
      }
      if (f->mirror && f->mirror->usable) descs[i].packed = f->mirror->data.as<char>();
      else if (f->n >= gp::kChunkPoints) all = false;
    }
    b->packed = all;
  }
  if (!b->packed)
    for (auto& d : descs) d.packed = nullptr;
  // tiles
  b->planned = fam == GP_KERNEL_STREAM && F == 1 && descs[0].n >= kPlanMinPoints;
  if (b->planned) {
    // one large factor: the balanced plan; the table holds the same tiles the in-argument launch derives from the plan (plan_tile)
    const int G = make_stream_plan(descs[0].n, b->tuning.balance, b->tuning.xcd_weights_set ? b->tuning.xcd_weights : nullptr, &b->plan, b->tuning.max_wgs);
    b->ppt = 4;
    b->tile_points = 0;
    descs[0].tile_begin = 0;
    for (int x = 0; x < gp::kNumXCD; x++)
      for (int q = 0; q < b->plan.wgs_per_xcd; q++) {
        int begin = 0, count = 0;
        gp::plan_tile(gp::plan_fields(b->plan, x, q), x, q, &begin, &count);
        tiles.push_back(gp::TileDesc{0, begin, count, (int)tiles.size()});
      }
    descs[0].tile_count = G;
  } else {
    int ppt = gp::kPipelineChunks;  // the hashed-line-table, reference-shaped and f64 kernels exist for 1024-point tiles only
    if (fam == GP_KERNEL_STREAM) {  // (round 6: the LOOKAHEAD family keeps its 1024-point tiles -- it exists for maps of >= 2^26 voxels, where no batch is small;
                                    //  its 512- / 256-point instantiations went with that: VERDICT r05 #8)
      // per batch: the largest tile that still fills 3/4 of the chip's resident workgroups, so that a 15 k-point scan is not left to 15 workgroups
      ppt = 1;
      for (int cand : {4, 2}) {
        int64_t count = 0;
        for (const auto* f : b->factors) count += (f->n + 256 * cand - 1) / (256 * cand);
        if (count >= kResidentWorkgroups * 3 / 4) {
          ppt = cand;
          break;
        }
      }
    }
    if (fam == GP_KERNEL_STREAM) {
      // the stream kernel takes tiles of any whole number of chunks: 2048-point tiles (eight chunks per wave: the cold start of the pipeline is paid
      // half as often) where that still leaves two rounds of workgroups -- C3 56.7 -> 51.3 us, C4 shard 135 -> 115 us, whole C4 1.08 -> 1.00 ms
      // (profiles/r03_tile_chunks.jsonl; 4096-point tiles: C3 54.7, C4 shard 114)
      int64_t count8 = 0;
      for (const auto* f : b->factors) count8 += (f->n + 2047) / 2048;
      if (count8 >= 2 * kResidentWorkgroups) ppt = 8;
      // ... and 4096-point tiles from 4096 such tiles up (a C4 shard: 512 factors x 8): with the factors finalized inside the tile kernel every tile ends with a
      // write-through row and an arrival, so fewer, larger tiles win while there are still four rounds of them (C4 shard 0.171 -> 0.163 ms; C3, 1536 such tiles: no)
      int64_t count16 = 0;
      for (const auto* f : b->factors) count16 += (f->n + 4095) / 4096;
      if (count16 >= 4 * kResidentWorkgroups) ppt = 16;
      if (b->tuning.tile_chunks > 0) ppt = b->tuning.tile_chunks;
    }
    b->ppt = ppt;
    b->tile_points = 64 * 4 * ppt;
    for (int i = 0; i < F; i++) {
      gp::FactorDesc& d = descs[i];
      d.tile_begin = (int)tiles.size();
      for (int t = 0, T = gp::fixed_tile_count(d.n, b->tile_points); t < T; t++) {
        int begin = 0, count = 0;
        gp::fixed_tile(t, d.n, b->tile_points, &begin, &count);
        tiles.push_back(gp::TileDesc{i, begin, count, (int)tiles.size()});
      }
      d.tile_count = (int)tiles.size() - d.tile_begin;
    }
  }
  b->num_tiles = (int)tiles.size();
  {
    std::vector<const float*> srcs;
    for (const auto& d : descs) srcs.push_back(d.points);
    std::sort(srcs.begin(), srcs.end());
    b->stream_once = b->shares_device_ok && std::adjacent_find(srcs.begin(), srcs.end()) == srcs.end();
    b->nt = b->tuning.source_policy == 2 || (b->tuning.source_policy == 0 && b->stream_once);
  }
  if (b->tuning.tile_interleave && !b->planned) {
    // execution order: consecutive factors that read the SAME source cloud (a submap matched against several targets, BASELINE
    // configs[3]) take turns tile by tile, so the workgroups that run side by side on an XCD read the same source bytes at the same
    // time -- one of them misses L2, the others hit.  Partial rows stay factor-major (TileDesc::row).
    std::vector<gp::TileDesc> order;
    order.reserve(tiles.size());
    for (int i = 0; i < F;) {
      int j = i + 1;
      while (j < F && descs[j].points == descs[i].points && descs[j].covs == descs[i].covs && descs[j].n == descs[i].n) j++;
      for (int t = 0; t < descs[i].tile_count; t++)
        for (int k = i; k < j; k++) order.push_back(tiles[(size_t)descs[k].tile_begin + t]);
      i = j;
    }
    tiles.swap(order);
  }
  b->h_descs = descs;
  GP_TRY(b->d_factors.ensure(sizeof(gp::FactorDesc) * (size_t)std::max(F, 1)));
  GP_TRY(b->d_tiles.ensure(sizeof(gp::TileDesc) * (size_t)std::max(b->num_tiles, 1)));
  GP_TRY(b->d_poses.ensure(sizeof(double) * 32 * (size_t)std::max(F, 1)));
  GP_TRY(b->h_poses.ensure(sizeof(double) * 32 * (size_t)std::max(F, 1)));
  GP_TRY(b->h_out.ensure(sizeof(gp_linearized6) * (size_t)std::max(F, kFinalizePartsMax)));
  GP_HIP(hipHostGetDevicePointer(&b->h_out_dev, b->h_out.ptr, 0));
  {
    const size_t before = b->h_done.bytes;
    GP_TRY(b->h_done.ensure(sizeof(unsigned long long) * (size_t)std::max(F, kFinalizePartsMax)));
    if (b->h_done.bytes != before) memset(b->h_done.ptr, 0, b->h_done.bytes);
    GP_HIP(hipHostGetDevicePointer(&b->h_done_dev, b->h_done.ptr, 0));
  }
  if (!b->temp_buffer) GP_TRY(b->d_partials.ensure(sizeof(double) * gp::ACCG_STRIDE * (size_t)std::max(b->num_tiles, 1)));
  // the table upload is synchronous (pageable source); it happens once per factor-set change, not per linearise
  if (F) GP_HIP(hipMemcpy(b->d_factors.ptr, descs.data(), sizeof(gp::FactorDesc) * (size_t)F, hipMemcpyHostToDevice));
  if (b->num_tiles) GP_HIP(hipMemcpy(b->d_tiles.ptr, tiles.data(), sizeof(gp::TileDesc) * (size_t)b->num_tiles, hipMemcpyHostToDevice));
  GP_TRY(measure_extents(b));
  b->seen.resize((size_t)F);
  for (int i = 0; i < F; i++) b->seen[i] = b->factors[i]->generation + b->factors[i]->target->generation;
  b->table_dirty = false;
  return GP_OK;
}

// the factor table caches device pointers: rebuild it when the tuning changed (set_tuning marks it dirty), a flag or source pointer of a
// factor changed, or a target map was re-inserted / offloaded / reloaded since (OffloadableGPU protocol)
bool table_is_stale(const gp_vgicp_batch* b) {
  if (b->table_dirty || b->seen.size() != b->factors.size()) return true;
  for (size_t i = 0; i < b->factors.size(); i++)
    if (b->seen[i] != b->factors[i]->generation + b->factors[i]->target->generation) return true;
  return false;
}

// is the 3x3 block of every pose orthonormal to 1e-9?  (gp::pose_is_rigid, gp_vgicp_shared.hpp)
bool poses_are_rigid(const double* poses_host, size_t F) {
  if (!poses_host) return false;
  for (size_t i = 0; i < F; i++)
    if (!gp::pose_is_rigid(poses_host + 16 * i)) return false;
  return true;
}

// does the batch (table built) take the 29-sum kernels + adjoint expansion at these poses?  Every 3x3 block orthonormal, and no pose FAR: the 29 sums are formed
// in f32 from q = R p + t, so H_t carries rounding of size |q|^2 M, and the expansion H_s = Ad^T H_t Ad (of size |p|^2 M) cancels about (|t| / |p|)^2 of it -- a
// scan registered against a map whose origin is kilometres away.  A pose with |t| > far_pose_ratio x the source's extent (largest |coordinate|) therefore takes the
// explicit-J_s sums like a non-orthonormal one (all f64, summed from p: nothing cancels).  Per call and per batch, like the orthonormality test.
bool takes_rigid_path(const gp_vgicp_batch* b, const double* poses_host) {
  const size_t F = b->factors.size();
  if (!poses_are_rigid(poses_host, F)) return false;
  const double ratio = (double)b->tuning.far_pose_ratio;
  if (ratio <= 0.0) return true;
  for (size_t i = 0; i < F; i++) {
    const gp_vgicp_factor* f = b->factors[i];
    if (f->n <= 0) continue;
    const double* t = poses_host + 16 * i + 12;
    const double lim = ratio * f->extent;
    if (t[0] * t[0] + t[1] * t[1] + t[2] * t[2] > lim * lim) return false;
  }
  return true;
}

// how long a synchronous call polls its completion words before it hands over to hipStreamSynchronize: 100 us + 50 ps per source point
// (4x what the tile kernel takes), so that a healthy pass never gets there
long spin_budget_us(const gp_vgicp_batch* b) { return 100 + (long)(b->total_points / 20000); }

// poses for a launch: a single factor carries them in the kernel arguments; a batch uploads them with one H2D
// zero_copy (the SYNCHRONOUS entry points, which return only after the kernels have finished): the kernels read the poses straight
// out of the pinned staging buffer over the fabric -- one 128-B scalar read per workgroup, hidden behind the other workgroups -- instead
// of behind a copy-engine transfer (an API call, an event and ~10 us of SDMA start-up in front of the first kernel).  The asynchronous
// issue_* entry points keep the H2D copy: the caller may re-stage poses while the kernels of the previous pass are still running.
int stage_poses(gp_vgicp_batch* b, const double* lin, const double* eval, PoseSource* ps, bool zero_copy = false) {
  const size_t F = b->factors.size();
  if (F == 1) {
    memcpy(ps->inl.lin, lin, sizeof(double) * 16);
    if (eval) memcpy(ps->inl.eval, eval, sizeof(double) * 16);
    ps->inl.factor = b->h_descs[0];
    ps->inl.tile_points = b->tile_points;
    ps->inl.use = 1;
    return GP_OK;
  }
  // the previous pass's H2D copy may still be reading the pinned staging buffer (the issue_* entry points are asynchronous):
  // wait for it before the buffer is overwritten
  if (b->h2d_done) {
    GP_HIP(hipEventSynchronize(b->h2d_done));
  } else {
    GP_HIP(hipEventCreateWithFlags(&b->h2d_done, hipEventDisableTiming));
  }
  double* h = b->h_poses.as<double>();
  memcpy(h, lin, sizeof(double) * 16 * F);
  if (eval) memcpy(h + 16 * F, eval, sizeof(double) * 16 * F);
  if (zero_copy) {
    void* hd = nullptr;
    GP_HIP(hipHostGetDevicePointer(&hd, h, 0));
    ps->d_lin = static_cast<const double*>(hd);
    ps->d_eval = eval ? static_cast<const double*>(hd) + 16 * F : nullptr;
    ps->inl.use = 0;
    return GP_OK;
  }
  GP_HIP(hipMemcpyAsync(b->d_poses.ptr, h, sizeof(double) * 16 * F * (eval ? 2 : 1), hipMemcpyHostToDevice, b->stream));
  GP_HIP(hipEventRecord(b->h2d_done, b->stream));
  ps->d_lin = b->d_poses.as<double>();
  ps->d_eval = eval ? b->d_poses.as<double>() + 16 * F : nullptr;
  ps->inl.use = 0;
  return GP_OK;
}

int ensure_self_batch(gp_vgicp_factor* f) {
  if (!f->self_batch) {
    // a batch of one on the factor's own stream whose partials live in the factor's TempBufferManager arena
    // (set before the table is built, so that no second partials array is allocated)
    auto* b = new gp_vgicp_batch;
    b->factors.push_back(f);
    b->stream = f->stream;
    b->temp_buffer = f->temp_buffer;
    b->tuning = f->tuning;
    const int rc = build_table(b);
    if (rc != GP_OK) {
      delete b;
      return rc;
    }
    f->self_batch = b;
  }
  if (table_is_stale(f->self_batch)) GP_TRY(build_table(f->self_batch));
  return GP_OK;
}

}  // namespace

// ---- the arrival protocol of the fused finalize ------------------------------------------------------------------------------------------------

// every synchronous call ends here: poll `count` completion words for `seq` (gp::wait_done), within the call's spin budget
static int wait_words(gp_vgicp_batch_t* b, size_t count, unsigned long long seq, long extra_spin_us = 0) {
  return gp::wait_done(static_cast<const unsigned long long*>(b->h_done.ptr), count, seq, b->stream, spin_budget_us(b) + extra_spin_us);
}

// gp_debug_drop_error_words: this fused error evaluation is to read as if its completion words had not arrived (host side only: the kernels run as always)
static bool take_dropped_error_words(gp_vgicp_batch_t* b) {
  if (b->drop_error_words <= 0) return false;
  b->drop_error_words--;
  return true;
}

// fused finalize: arrival counters (monotonic, one per part, kArriveStride words apart) and where the parts' last workgroups deliver
static int arm_arrival(gp_vgicp_batch_t* b, PoseSource* ps, int parts, int per, const gp::DoneFlags& done) {
  if (!b->d_arrive.ptr) {
    GP_TRY(b->d_arrive.alloc(sizeof(unsigned long long) * 16 * gp::kArriveStride));
    GP_HIP(hipMemset(b->d_arrive.ptr, 0, sizeof(unsigned long long) * 16 * gp::kArriveStride));
    memset(b->arrived, 0, sizeof(b->arrived));
  }
  ps->inl.arrive = b->d_arrive.as<unsigned long long>();
  ps->inl.rows_per_part = per;
  ps->inl.num_rows = b->num_tiles;
  for (int g = 0; g < parts; g++)  // (committed to b->arrived by fused_launched() once the launch has gone out)
    ps->inl.arrive_target[g] = b->arrived[g] + (unsigned long long)std::max(0, std::min(per, b->num_tiles - g * per));
  ps->inl.fin_out = static_cast<double*>(b->h_out_dev);
  ps->inl.fin_stride = (int)(sizeof(gp_linearized6) / sizeof(double));
  ps->inl.fin_flags = done.flags;
  ps->inl.fin_seq = done.seq;
  return GP_OK;
}

static void fused_launched(gp_vgicp_batch_t* b, const PoseSource& ps, int parts) {
  for (int g = 0; g < parts; g++) b->arrived[g] = ps.inl.arrive_target[g];
}
// did every part's completion word arrive?  (after wait_done, which hands over to hipStreamSynchronize when its spin budget is used up: in the two-kernel
// form a finished stream means finished records, in the fused form the records exist only if the parts' last workgroups saw their counters complete)
static bool words_arrived(const gp_vgicp_batch_t* b, int count, unsigned long long seq) {
  const volatile unsigned long long* fl = static_cast<const volatile unsigned long long*>(b->h_done.ptr);
  for (int g = 0; g < count; g++)
    if (fl[g] != seq) return false;
  return true;
}

// The by-factor fused finalize counts arrivals in zero-reset counters (the last arriver of a factor stores 0): a launch that went out and was never seen to complete
// (an error return between launch and the last completion word, a torn-down kernel) may have left small positive values behind, which would let the NEXT launch's
// factors finalize early on stale rows without anybody noticing.  Such a batch cleans its counters, behind the stream, before it counts again.
static int clean_factor_arrivals(gp_vgicp_batch_t* b) {
  if (!b->factor_arrive_dirty || !b->d_factor_arrive.ptr) return GP_OK;
  GP_HIP(hipStreamSynchronize(b->stream));
  GP_HIP(hipMemset(b->d_factor_arrive.ptr, 0, sizeof(unsigned long long) * gp::kFactorArriveStride * b->factor_arrive_count));
  b->factor_arrive_dirty = false;
  return GP_OK;
}

// fused finalize by FACTOR: ONE launch, the workgroup that stores a factor's last row finalizes the factor (gp_vgicp_stream.hpp) and hands slot i of fin_out (fin_stride
// doubles apart: a record, or one double of an error evaluation) and completion word i to the host.  One zero-reset counter per factor; *partials = the launch's rows.
// factor_arrive_dirty stays set until the caller has seen every completion word of THIS launch: an error return in between leaves it set.
static int arm_factor_arrival(gp_vgicp_batch_t* b, PoseSource* ps, int fin_stride, const gp::DoneFlags& done, double** partials) {
  const size_t F = b->factors.size();
  if (b->factor_arrive_count < F) {
    const size_t bytes = sizeof(unsigned long long) * gp::kFactorArriveStride * F;
    GP_TRY(b->d_factor_arrive.alloc(bytes));
    GP_HIP(hipMemset(b->d_factor_arrive.ptr, 0, bytes));
    b->factor_arrive_count = F;
  }
  GP_TRY(partials_ptr(b, partials));
  GP_TRY(clean_factor_arrivals(b));
  ps->inl.arrive = b->d_factor_arrive.as<unsigned long long>();
  ps->inl.rows_per_part = 0;
  ps->inl.num_rows = b->num_tiles;
  ps->inl.fin_out = static_cast<double*>(b->h_out_dev);
  ps->inl.fin_stride = fin_stride;
  ps->inl.fin_flags = done.flags;
  ps->inl.fin_seq = done.seq;
  b->factor_arrive_dirty = true;
  return GP_OK;
}

// ... a factor without points has no workgroup to finalize it: its slot and its completion word are written here.  poses_host: the linearise's poses (the empty
// record is the expansion of zero sums at the factor's pose); null: an error evaluation (the empty sum)
static void write_empty_factors(gp_vgicp_batch_t* b, const double* poses_host, unsigned long long seq) {
  for (size_t i = 0; i < b->factors.size(); i++)
    if (b->h_descs[i].tile_count == 0) {
      if (poses_host) {
        const double zeros[32] = {0.0};
        expand_rigid_host(zeros, poses_host + 16 * i, reinterpret_cast<double*>(static_cast<gp_linearized6*>(b->h_out.ptr) + i));
      } else {
        static_cast<volatile double*>(b->h_out.ptr)[i] = 0.0;
      }
      static_cast<volatile unsigned long long*>(b->h_done.ptr)[i] = seq;
    }
}

// The stream is idle and completion words of a fused launch are missing: the device's counters and the host's idea of them have come apart (a launch that failed
// half way, a kernel that was torn down, a counter left dirty).  The rows are complete, so the counters of that form start over from zero and the call's sums are
// done again in the two-kernel form, which announces itself with the words returned here.
static int recover_arrival(gp_vgicp_batch_t* b, bool by_factor, gp::DoneFlags* again) {
  if (by_factor) {
    GP_HIP(hipMemset(b->d_factor_arrive.ptr, 0, sizeof(unsigned long long) * gp::kFactorArriveStride * b->factors.size()));
  } else {
    GP_HIP(hipStreamSynchronize(b->stream));
    if (b->d_arrive.ptr) GP_HIP(hipMemset(b->d_arrive.ptr, 0, sizeof(unsigned long long) * 16 * gp::kArriveStride));
    memset(b->arrived, 0, sizeof(b->arrived));
  }
  *again = gp::DoneFlags{static_cast<unsigned long long*>(b->h_done_dev), ++b->seq, nullptr};
  return GP_OK;
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
  if (table_is_stale(b)) GP_TRY(build_table(b));
  PoseSource ps;
  GP_TRY(stage_poses(b, poses_host, nullptr, &ps, true));
  const gp::DoneFlags done{static_cast<unsigned long long*>(b->h_done_dev), ++b->seq, b->trace ? b->trace + 2047 * 16 : nullptr};
  const bool rigid = takes_rigid_path(b, poses_host);
  const int parts = (F == 1 && rigid && b->num_tiles >= kFinalizeSplitTiles) ? kFinalizeParts : 1;
  const bool sums_only = parts > 1;  // the parts deliver their 32 sums, the host expands once (the parts expanding: measured slower, round 2)
  if (b->timing && !b->ev[0])
    for (auto& e : b->ev) GP_HIP(hipEventCreate(&e));
  const bool fused = sums_only && b->family == GP_KERNEL_STREAM && ps.inl.use && b->tuning.fused_finalize && !b->timing;
  if (fused) {
    // ONE launch: the last workgroup of each part of the tile list finalizes the part (gp_vgicp_stream.hpp: finalize_part_rows)
    double* partials = nullptr;
    GP_TRY(partials_ptr(b, &partials));
    GP_TRY(arm_arrival(b, &ps, parts, (b->num_tiles + parts - 1) / parts, done));
    GP_TRY(launch_tiles<gp::MODE_LIN>(b, ps, partials));
    fused_launched(b, ps, parts);
    GP_TRY(wait_words(b, (size_t)parts, done.seq));
    if (!words_arrived(b, parts, done.seq)) {  // the finalize kernel does this call's sums
      gp::DoneFlags again;
      GP_TRY(recover_arrival(b, false, &again));
      GP_TRY(launch_finalize<false>(b, ps, partials, reinterpret_cast<gp_linearized6*>(b->h_out_dev), again, -parts));
      GP_TRY(wait_words(b, (size_t)parts, again.seq));
    } else {
      // the step as the device saw it: first workgroup started .. last row in .. last sums out (words 34 / 32 / 33 of the parts' slots)
      const unsigned long long* w = static_cast<const unsigned long long*>(b->h_out.ptr);
      constexpr size_t N = sizeof(gp_linearized6) / sizeof(double);
      unsigned long long t0 = ~0ull, t_rows = 0, t_out = 0;
      for (int g = 0; g < parts; g++) {
        if (g < gp::kNumXCD) t0 = std::min(t0, w[g * N + 34]);
        t_rows = std::max(t_rows, w[g * N + 32]);
        t_out = std::max(t_out, w[g * N + 33]);
      }
      if (t0 <= t_rows && t_rows <= t_out && t_out - t0 < 100000000ull) {
        b->dev_steps += 1.0;
        b->dev_stream_ticks += (double)(t_rows - t0);
        b->dev_kernel_ticks += (double)(t_out - t0);
      }
    }
  } else if (parts == 1 && rigid && b->family == GP_KERNEL_STREAM && b->tuning.fused_finalize && !b->timing && !b->trace) {
    // ONE launch for a batch (or a small single factor): the workgroup that stores a factor's last row finalizes the factor (gp_vgicp_stream.hpp), so
    // the records leave for the host while the other factors' tiles are still running
    double* partials = nullptr;
    GP_TRY(arm_factor_arrival(b, &ps, (int)(sizeof(gp_linearized6) / sizeof(double)), done, &partials));
    GP_TRY(launch_tiles<gp::MODE_LIN>(b, ps, partials));
    write_empty_factors(b, poses_host, done.seq);
    GP_TRY(wait_words(b, F, done.seq));
    if (!words_arrived(b, (int)F, done.seq)) {  // the finalize kernel does this call's records
      gp::DoneFlags again;
      GP_TRY(recover_arrival(b, true, &again));
      ps.inl.arrive = nullptr;
      GP_TRY(launch_finalize<false>(b, ps, partials, reinterpret_cast<gp_linearized6*>(b->h_out_dev), again, 1));
      GP_TRY(wait_words(b, F, again.seq));
    }
    b->factor_arrive_dirty = false;  // every factor's last arriver reset its counter (or the fallback cleaned them)
  } else {
    GP_TRY(launch_linearize(b, ps, reinterpret_cast<gp_linearized6*>(b->h_out_dev), rigid, done, sums_only ? -parts : parts, b->timing));
    GP_TRY(wait_words(b, F * (size_t)parts, done.seq));
  }
  if (b->timing) {  // measurement: the two kernels of THIS synchronous pass, i.e. behind the idle queue the host left between two passes
    GP_HIP(hipEventSynchronize(b->ev[2]));
    GP_HIP(hipEventElapsedTime(&b->last_tile_ms, b->ev[0], b->ev[1]));
    GP_HIP(hipEventElapsedTime(&b->last_finalize_ms, b->ev[1], b->ev[2]));
  }
  if (parts == 1) {
    if (view) *view = static_cast<const gp_linearized6*>(b->h_out.ptr);
    if (out_host && !(view && F == 1)) memcpy(out_host, b->h_out.ptr, sizeof(gp_linearized6) * F);
  } else {
    if (view) *view = out_host;  // F == 1: caller's array or view_store
    const double* p = static_cast<const double*>(b->h_out.ptr);
    double* o = reinterpret_cast<double*>(out_host);
    constexpr int N = (int)(sizeof(gp_linearized6) / sizeof(double));
    // the parts' 32 sums add up in slot order; one expansion on the host
    double total[32];
    for (int k = 0; k < 32; k++) {
      double a = p[k];
      for (int q = 1; q < parts; q++) a += p[(size_t)q * N + k];
      total[k] = a;
    }
    expand_rigid_host(total, poses_host, o);
  }
  return GP_OK;
}

extern "C" {

// ---- per-batch tuning (nothing process-global: SURVEY.md 8(b) "re-entrant across handles") --------------------------------------------------
static int apply_tuning(gp_vgicp_tuning* t, int key, int value) {
  switch (key) {
    case GP_TUNE_KERNEL:
      if (value != GP_KERNEL_REFERENCE && value != GP_KERNEL_HASHED && value != GP_KERNEL_GRID_F64 && value != GP_KERNEL_LOOKAHEAD && value != GP_KERNEL_STREAM)
        return gp::fail(GP_ERROR_INVALID_ARGUMENT, "GP_TUNE_KERNEL: one of GP_KERNEL_REFERENCE (0), _HASHED (2), _GRID_F64 (3), _LOOKAHEAD (8), _STREAM (12)");
      t->kernel = value;
      return GP_OK;
    case GP_TUNE_SOURCE_POLICY:
      if (value < 0 || value > 2) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "GP_TUNE_SOURCE_POLICY: 0 (per batch), 1 (default cache policy), 2 (non-temporal)");
      t->source_policy = value;
      return GP_OK;
    case GP_TUNE_XCD_CHUNK:
      if (value < 0 || value > 4096) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "GP_TUNE_XCD_CHUNK: 0 (contiguous eighths) .. 4096 tiles per run");
      t->xcd_chunk = value;
      return GP_OK;
    case GP_TUNE_STAGGER:
      if (value < 0 || value > 64) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "GP_TUNE_STAGGER: 0..64 (x 512 clocks)");
      t->stagger = value;
      return GP_OK;
    case GP_TUNE_TILE_INTERLEAVE:
      t->tile_interleave = value ? 1 : 0;
      return GP_OK;
    case GP_TUNE_FUSED_FINALIZE:
      t->fused_finalize = value ? 1 : 0;
      return GP_OK;
    case GP_TUNE_MAX_WORKGROUPS:
      if (value < 8 || value > 1024) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "GP_TUNE_MAX_WORKGROUPS: 8 .. 1024");
      t->max_wgs = value;
      return GP_OK;
    case GP_TUNE_TILE_CHUNKS:
      if (value < 0 || value > 64) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "GP_TUNE_TILE_CHUNKS: 0 (automatic) .. 64 chunks per wave");
      t->tile_chunks = value;
      return GP_OK;
    case GP_TUNE_SOURCE_MIRROR:
      t->source_mirror = value ? 1 : 0;
      return GP_OK;
    case GP_TUNE_FAR_POSE_RATIO:
      if (value < 0 || value > 1000000) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "GP_TUNE_FAR_POSE_RATIO: 0 (no pose counts as far) .. 1000000 (x the source cloud's extent)");
      t->far_pose_ratio = value;
      return GP_OK;
    case GP_TUNE_BALANCE:
      // make_stream_plan refuses a skew that overdraws an XCD's share and deals that launch flat
      if (value < -1 || value > 1000) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "GP_TUNE_BALANCE: -1 (automatic), 0 (flat) .. 1000 (per mille of the mean share per dispatch round)");
      t->balance = value;
      return GP_OK;
    default:
      if (key >= GP_TUNE_XCD_WEIGHT_0 && key < GP_TUNE_XCD_WEIGHT_0 + 8) {
        if (value < 500 || value > 1500) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "GP_TUNE_XCD_WEIGHT_x: 500..1500 (per mille of the mean share)");
        t->xcd_weights[key - GP_TUNE_XCD_WEIGHT_0] = value;
        t->xcd_weights_set = true;
        return GP_OK;
      }
      return gp::fail(GP_ERROR_INVALID_ARGUMENT, "unknown GP_TUNE_* key");
  }
}

int gp_vgicp_batch_set_tuning(gp_vgicp_batch_t* b, int key, int value) {
  if (!b) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_set_tuning: null batch");
  if (key == GP_TUNE_TIMING) {
    b->timing = value != 0;
    return GP_OK;
  }
  if (key == GP_TUNE_TEST_ARRIVAL_SKEW) {  // test hook: the host's idea of arrival counter 0 runs `value` ahead of the device's, as after a launch that was lost
    b->arrived[0] += (unsigned long long)(value > 0 ? value : 0);
    if (b->d_factor_arrive.ptr && value > 0) {  // ... and factor counter 0 is far out of range: that factor's record cannot complete
      const unsigned long long v = 1ull << 40;
      GP_HIP(hipStreamSynchronize(b->stream));
      GP_HIP(hipMemcpy(b->d_factor_arrive.ptr, &v, sizeof(v), hipMemcpyHostToDevice));
    }
    return GP_OK;
  }
  GP_TRY(apply_tuning(&b->tuning, key, value));
  b->table_dirty = true;
  return GP_OK;
}

int gp_vgicp_batch_get_tuning(const gp_vgicp_batch_t* b, int key, int* value) {
  if (!b || !value) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_get_tuning: null");
  switch (key) {
    case GP_TUNE_KERNEL: *value = b->tuning.kernel; return GP_OK;
    case GP_TUNE_SOURCE_POLICY: *value = b->tuning.source_policy; return GP_OK;
    case GP_TUNE_XCD_CHUNK: *value = b->tuning.xcd_chunk; return GP_OK;
    case GP_TUNE_STAGGER: *value = b->tuning.stagger; return GP_OK;
    case GP_TUNE_TILE_INTERLEAVE: *value = b->tuning.tile_interleave; return GP_OK;
    case GP_TUNE_BALANCE: *value = b->tuning.balance; return GP_OK;
    case GP_TUNE_FUSED_FINALIZE: *value = b->tuning.fused_finalize; return GP_OK;
    case GP_TUNE_TILE_CHUNKS: *value = b->tuning.tile_chunks; return GP_OK;
    case GP_TUNE_EFFECTIVE_KERNEL: *value = b->table_dirty ? -1 : b->family; return GP_OK;  // what the last table build resolved GP_TUNE_KERNEL to
    case GP_TUNE_SOURCE_MIRROR: *value = b->tuning.source_mirror; return GP_OK;
    case GP_TUNE_FAR_POSE_RATIO: *value = b->tuning.far_pose_ratio; return GP_OK;
    case GP_TUNE_EFFECTIVE_MIRROR: *value = b->table_dirty ? -1 : (b->packed ? 1 : 0); return GP_OK;  // does the built table stream the packed mirrors?
    default: return gp::fail(GP_ERROR_INVALID_ARGUMENT, "unknown GP_TUNE_* key");
  }
}

// the per-factor entry points run a batch of one: its tuning is the factor's
int gp_vgicp_factor_set_tuning(gp_vgicp_factor_t* f, int key, int value) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_factor_set_tuning: null factor");
  GP_TRY(apply_tuning(&f->tuning, key, value));
  if (f->self_batch) {
    f->self_batch->tuning = f->tuning;
    f->self_batch->table_dirty = true;
  }
  return GP_OK;
}

// timeline hook (measurement): the traced build of the tile kernel of THIS batch's single-factor linearise stores 8 s_memtime stamps + HW_ID /
// XCC_ID + two s_memrealtime stamps per workgroup into dev_buffer ([2048][16] uint64, row = tile index); row 2047 receives the stamps of the
// finalize kernel of synchronous calls.  NULL disables.
int gp_vgicp_batch_set_trace_buffer(gp_vgicp_batch_t* b, void* dev_buffer) {
  if (!b) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_set_trace_buffer: null batch");
  b->trace = static_cast<unsigned long long*>(dev_buffer);
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
  if (pose_host) {  // the host copy rides in the kernel arguments; the device copy is not even read
    memcpy(ps.inl.lin, pose_host, sizeof(double) * 16);
    ps.inl.factor = f->self_batch->h_descs[0];
    ps.inl.tile_points = f->self_batch->tile_points;
    ps.inl.use = 1;
  } else {
    ps.d_lin = pose_dev;
  }
  return launch_linearize(f->self_batch, ps, out_dev, takes_rigid_path(f->self_batch, pose_host));
}

int gp_vgicp_factor_issue_compute_error(gp_vgicp_factor_t* f, const double* pose_lin_host, const double* pose_eval_host, const double* pose_lin_dev,
                                        const double* pose_eval_dev, double* out_dev) {
  if (!f || !out_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_factor_issue_compute_error: null");
  GP_TRY(ensure_self_batch(f));
  PoseSource ps;
  if (pose_lin_host && pose_eval_host) {
    memcpy(ps.inl.lin, pose_lin_host, sizeof(double) * 16);
    memcpy(ps.inl.eval, pose_eval_host, sizeof(double) * 16);
    ps.inl.factor = f->self_batch->h_descs[0];
    ps.inl.tile_points = f->self_batch->tile_points;
    ps.inl.use = 1;
  } else if (pose_lin_dev && pose_eval_dev) {
    ps.d_lin = pose_lin_dev;
    ps.d_eval = pose_eval_dev;
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
  int rc = build_table(b);
  if (rc != GP_OK) {
    delete b;
    return rc;
  }
  *out = b;
  return GP_OK;
}

// gp_multi.hip: several shards of one multi-batch run on this device and read the same source clouds one after the other, so the source
// stream of this batch must stay cacheable (no non-temporal policy)
extern "C++" {
namespace gp {
void batch_set_sources_shared(gp_vgicp_batch* batch, bool shared) {
  if (!batch || batch->shares_device_ok == !shared) return;
  batch->shares_device_ok = !shared;
  batch->table_dirty = true;
}
}  // namespace gp
}

// measurement: durations of the tile kernel and the finalize kernel of the last synchronous linearise (GP_TUNE_TIMING = 1), HIP events on the batch's stream
int gp_vgicp_batch_device_times(gp_vgicp_batch_t* batch, int reset, double* steps, double* stream_us_mean, double* kernel_us_mean) {
  if (!batch) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_device_times: null batch");
  if (steps) *steps = batch->dev_steps;
  if (stream_us_mean) *stream_us_mean = batch->dev_steps > 0 ? batch->dev_stream_ticks / batch->dev_steps / 100.0 : 0.0;
  if (kernel_us_mean) *kernel_us_mean = batch->dev_steps > 0 ? batch->dev_kernel_ticks / batch->dev_steps / 100.0 : 0.0;
  if (reset) batch->dev_steps = batch->dev_stream_ticks = batch->dev_kernel_ticks = 0.0;
  return GP_OK;
}

int gp_vgicp_batch_last_kernel_ms(const gp_vgicp_batch_t* batch, float* tile_ms, float* finalize_ms) {
  if (!batch) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_last_kernel_ms: null batch");
  if (tile_ms) *tile_ms = batch->last_tile_ms;
  if (finalize_ms) *finalize_ms = batch->last_finalize_ms;
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

int64_t gp_vgicp_batch_algorithmic_bytes(const gp_vgicp_batch_t* batch) {
  if (!batch) return 0;
  int64_t bytes = 0;
  for (const auto* f : batch->factors)
    bytes += 48ll * f->n + 16ll * f->target->info.num_buckets + 52ll * f->target->info.num_voxels + 560ll + (f->surface_validation ? 12ll * f->n : 0ll);
  return bytes;
}

// what one pass of the batch's built table really requests from memory with perfect reuse of the lookup structures: the source stream as the kernel reads it
// (36 B per point through the packed mirrors, else 48; + 12 with surface validation), every DISTINCT map's block grid (16 B per 4x4x4 voxels of its box) or
// bucket table and its 64-B records once, pose in and record out.  Beside gp_vgicp_batch_algorithmic_bytes (the reference-layout accounting,
// which repacking does not change) in bench.py's roofline object.
int64_t gp_vgicp_batch_actual_bytes(gp_vgicp_batch_t* batch) {
  if (!batch) return 0;
  if (table_is_stale(batch) && build_table(batch) != GP_OK) return 0;
  int64_t bytes = 0;
  std::vector<const gp_voxelmap*> maps;
  for (const auto* f : batch->factors) {
    const int full = batch->packed ? f->n / gp::kChunkPoints * gp::kChunkPoints : 0;  // (the points behind the last full chunk come from the caller's arrays)
    bytes += 36ll * full + 48ll * (f->n - full) + 560ll + (f->surface_validation && f->normals ? 12ll * f->n : 0ll);
    if (std::find(maps.begin(), maps.end(), f->target) == maps.end()) maps.push_back(f->target);
  }
  for (const auto* m : maps)
    bytes += 64ll * m->info.num_voxels + (m->has_grid && batch->use_grid ? 16ll * m->num_grid_blocks() : 16ll * m->info.num_buckets);
  return bytes;
}

int gp_vgicp_batch_issue_linearize(gp_vgicp_batch_t* b, const double* poses_host, gp_linearized6* out_dev) {
  if (!b || !poses_host || !out_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_issue_linearize: null");
  if (table_is_stale(b)) GP_TRY(build_table(b));
  if (b->factors.empty()) return GP_OK;
  PoseSource ps;
  GP_TRY(stage_poses(b, poses_host, nullptr, &ps));
  return launch_linearize(b, ps, out_dev, takes_rigid_path(b, poses_host));
}

// which kernels the host-pose entry points run at these poses: 1 = the 29 sums + adjoint expansion (every 3x3 block orthonormal to 1e-9, no pose far from its
// source cloud: takes_rigid_path), 0 = the explicit-J_s sums.  What a caller of gp_vgicp_batch_issue_linearize_dev passes as `rigid` to choose the same.
int gp_vgicp_batch_takes_rigid_path(gp_vgicp_batch_t* b, const double* poses_host, int* out) {
  if (!b || !poses_host || !out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_takes_rigid_path: null");
  if (table_is_stale(b)) GP_TRY(build_table(b));
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
  if (table_is_stale(b)) GP_TRY(build_table(b));
  if (b->factors.empty()) return GP_OK;
  PoseSource ps;
  GP_TRY(stage_poses(b, poses_lin_host, poses_eval_host, &ps));
  return launch_error(b, ps, out_dev);
}

// the same two passes with the poses ALREADY in device memory (double[F][16] per table, column-major -- what a device-side retract produces, gp_lm.hip): no staging,
// no H2D copy, nothing for the host to wait on before the next call.  rigid: the caller vouches that every 3x3 block is orthonormal to 1e-9 (what the host-pose entry
// points test for themselves, poses_are_rigid): the 29-sum kernel + adjoint expansion; 0 = the 92-sum kernel, exact for any 3x3 block.  Any F (a single factor reads its descriptor and pose from the
// tables like the batch's other members: the in-argument form needs the pose on the host).
int gp_vgicp_batch_issue_linearize_dev(gp_vgicp_batch_t* b, const double* poses_dev, int rigid, gp_linearized6* out_dev) {
  if (!b || !poses_dev || !out_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_issue_linearize_dev: null");
  if (table_is_stale(b)) GP_TRY(build_table(b));
  if (b->factors.empty()) return GP_OK;
  PoseSource ps;
  ps.d_lin = poses_dev;
  ps.inl.use = 0;
  // (the by-factor fused finalize of the synchronous call was tried here too -- records written by the factors' last tile workgroups, no finalize launch -- and measured
  //  4 us SLOWER on BASELINE configs[2]'s batch: 59 us against 49.6 + 5.0, the 256 factors' tails end later than one finalize kernel over all of them; the error
  //  evaluation below keeps its fused form: 52 us against 49.5 + 9.2)
  return launch_linearize(b, ps, out_dev, rigid != 0);
}

int gp_vgicp_batch_issue_compute_error_dev(gp_vgicp_batch_t* b, const double* poses_lin_dev, const double* poses_eval_dev, double* out_dev) {
  if (!b || !poses_lin_dev || !poses_eval_dev || !out_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_issue_compute_error_dev: null");
  if (table_is_stale(b)) GP_TRY(build_table(b));
  if (b->factors.empty()) return GP_OK;
  PoseSource ps;
  ps.d_lin = poses_lin_dev;
  ps.d_eval = poses_eval_dev;
  ps.inl.use = 0;
  return launch_error(b, ps, out_dev);
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
  if (table_is_stale(b)) GP_TRY(build_table(b));
  if (b->factors.empty()) return GP_OK;
  PoseSource ps;
  ps.d_lin = poses_lin_dev;
  ps.d_eval = poses_eval_dev;
  ps.inl.use = 0;
  const gp::DoneFlags done{static_cast<unsigned long long*>(b->h_done_dev), ++b->seq};
  b->dev_error_fused = false;
  if (b->family == GP_KERNEL_STREAM && b->tuning.fused_finalize && !b->trace && !b->planned) {
    // ONE launch, as the synchronous call's by-factor form (gp_vgicp_batch_compute_error): the factor's last tile workgroup adds its rows up and hands sum and word over
    double* partials = nullptr;
    GP_TRY(arm_factor_arrival(b, &ps, 1, done, &partials));
    GP_TRY(launch_tiles<gp::MODE_ERR>(b, ps, partials));
    write_empty_factors(b, nullptr, done.seq);
    b->dev_error_fused = true;
    b->dev_error_lin = poses_lin_dev, b->dev_error_eval = poses_eval_dev;
    return GP_OK;
  }
  return launch_error(b, ps, static_cast<double*>(b->h_out_dev), done);
}

int gp_vgicp_batch_compute_error_dev_end(gp_vgicp_batch_t* b, double* out_host) {
  if (!b || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_compute_error_dev_end: null");
  const size_t F = b->factors.size();
  if (F == 0) return GP_OK;
  GP_TRY(wait_words(b, F, b->seq, 400));  // (+ the damped step queued in front of it)
  if (b->dev_error_fused) {
    const bool dropped = take_dropped_error_words(b);
    if (dropped || !words_arrived(b, (int)F, b->seq)) {  // (as gp_vgicp_batch_compute_error: a counter left dirty by a launch that did not run to its end)
      // Unlike the synchronous call, the rows of the pass cannot be summed again here: work queued behind _begin on the batch's stream -- gp_lm.hip's speculative
      // linearise -- writes the same partials buffer.  So the pass runs again in its two-kernel form (tile kernel + vgicp_finalize_error_kernel, the order of sums
      // the fused form keeps) at the poses _begin was given, behind everything queued so far.
      GP_HIP(hipStreamSynchronize(b->stream));
      gp::DoneFlags again;
      GP_TRY(recover_arrival(b, true, &again));
      PoseSource ps;
      ps.d_lin = b->dev_error_lin;
      ps.d_eval = b->dev_error_eval;
      ps.inl.use = 0;
      GP_TRY(launch_error(b, ps, static_cast<double*>(b->h_out_dev), again));
      GP_TRY(wait_words(b, F, again.seq));
    }
    b->factor_arrive_dirty = false;
    b->dev_error_fused = false;
  }
  memcpy(out_host, b->h_out.ptr, sizeof(double) * F);
  return GP_OK;
}

int gp_debug_drop_error_words(gp_vgicp_batch_t* b, int count) {
  if (!b || count < 0) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_debug_drop_error_words: a batch and count >= 0");
  b->drop_error_words = count;
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

// host-side check hook (no device needed): the tiles a planned single-factor launch of n points deals to its workgroups, in tile-list order
// (XCD-major).  begin / count: arrays of `capacity` ints; *num_tiles = workgroups of the launch (<= 1024).
int gp_debug_stream_plan(int n, int skew_permille, const int* xcd_weights_permille, int capacity, int* begin, int* count, int* num_tiles) {
  if (n < 0 || skew_permille < -1 || !num_tiles) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_debug_stream_plan: bad arguments");
  gp::StreamPlan plan;
  const int G = make_stream_plan(n, skew_permille, xcd_weights_permille, &plan);
  *num_tiles = G;
  if (begin && count) {
    if (capacity < G) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_debug_stream_plan: capacity too small");
    int t = 0;
    for (int x = 0; x < gp::kNumXCD; x++)
      for (int q = 0; q < plan.wgs_per_xcd; q++, t++) gp::plan_tile(gp::plan_fields(plan, x, q), x, q, &begin[t], &count[t]);
  }
  return GP_OK;
}

// ... the same with the launch's other inputs, down to the waves.  tile_points == 0: the planned launch of at most max_workgroups workgroups (GP_TUNE_MAX_WORKGROUPS;
// make_stream_plan + plan_tile, what build_table() stores and the kernel derives); tile_points > 0: the fixed tiles of a small factor (a whole number of chunks per
// wave).  waves, if given: [capacity * 4][3] = first point, full chunks and tail of every wave of every workgroup (split_tile, the kernel's own function).
int gp_debug_stream_plan_ex(int n, int tile_points, int max_workgroups, int skew_permille, const int* xcd_weights_permille, int capacity, int* begin, int* count,
                            long long* waves, int* num_tiles) {
  if (n < 0 || skew_permille < -1 || !num_tiles || tile_points < 0 || tile_points % (4 * gp::kChunkPoints) != 0 || (tile_points == 0 && (max_workgroups < 8 || max_workgroups > 1024)))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_debug_stream_plan_ex: bad arguments");
  gp::StreamPlan plan;
  const int G = tile_points ? gp::fixed_tile_count(n, tile_points) : make_stream_plan(n, skew_permille, xcd_weights_permille, &plan, max_workgroups);
  *num_tiles = G;
  if (!begin || !count) return GP_OK;
  if (capacity < G) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_debug_stream_plan_ex: capacity too small");
  if (tile_points) {
    for (int t = 0; t < G; t++) gp::fixed_tile(t, n, tile_points, &begin[t], &count[t]);
  } else {
    int t = 0;
    for (int x = 0; x < gp::kNumXCD; x++)
      for (int q = 0; q < plan.wgs_per_xcd; q++, t++) gp::plan_tile(gp::plan_fields(plan, x, q), x, q, &begin[t], &count[t]);
  }
  if (waves)
    for (int t = 0; t < G; t++)
      for (int w = 0; w < 4; w++) {
        const gp::WaveWork ww = gp::split_tile(begin[t], count[t], w);
        long long* o = waves + ((size_t)t * 4 + w) * 3;
        o[0] = (long long)ww.first, o[1] = ww.n, o[2] = ww.tail;
      }
  return GP_OK;
}

// host-side check hook (no device needed): the expansion the synchronous single-factor call runs on the added sums of its finalize parts
int gp_debug_expand_rigid(const double sums[32], const double pose[16], gp_linearized6* out) {
  if (!sums || !pose || !out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_debug_expand_rigid: null");
  expand_rigid_host(sums, pose, reinterpret_cast<double*>(out));
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
  if (table_is_stale(b)) GP_TRY(build_table(b));
  PoseSource ps;
  GP_TRY(stage_poses(b, poses_lin_host, poses_eval_host, &ps, true));
  const gp::DoneFlags done{static_cast<unsigned long long*>(b->h_done_dev), ++b->seq};
  const int parts = (F == 1 && ps.inl.use && b->family == GP_KERNEL_STREAM && b->num_tiles >= kFinalizeSplitTiles) ? kFinalizeParts : 1;
  if (parts > 1) {
    // one large factor: eight part sums, added here in slot order -- by the part's last tile workgroup (fused, one launch) or by a second kernel
    double* partials = nullptr;
    GP_TRY(partials_ptr(b, &partials));
    const int per = (b->num_tiles + parts - 1) / parts;
    constexpr int kSlot = (int)(sizeof(gp_linearized6) / sizeof(double));
    gp::DoneFlags second = done;  // what the second kernel of the two-kernel form announces itself with
    bool need_second = true;
    if (b->tuning.fused_finalize) {
      GP_TRY(arm_arrival(b, &ps, parts, per, done));
      GP_TRY(launch_tiles<gp::MODE_ERR>(b, ps, partials));
      fused_launched(b, ps, parts);
      GP_TRY(wait_words(b, (size_t)parts, done.seq));
      const bool dropped = take_dropped_error_words(b);
      if (dropped || !words_arrived(b, parts, done.seq)) {  // (see batch_linearize_sync)
        GP_TRY(recover_arrival(b, false, &second));
      } else {
        need_second = false;
      }
    } else {
      GP_TRY(launch_tiles<gp::MODE_ERR>(b, ps, partials));
    }
    if (need_second) {
      GP_TRY(gp::launch_finalize_error_parts(b->stream, partials, b->num_tiles, per, parts, static_cast<double*>(b->h_out_dev), kSlot, second));
      GP_TRY(wait_words(b, (size_t)parts, second.seq));
    }
    const double* p = static_cast<const double*>(b->h_out.ptr);
    double a = p[0];
    for (int q = 1; q < parts; q++) a += p[(size_t)q * kSlot];
    out_host[0] = a;
    return GP_OK;
  }
  if (b->family == GP_KERNEL_STREAM && b->tuning.fused_finalize && !b->trace) {
    // ONE launch (round 4): the workgroup that stores a factor's last row adds the factor's rows up -- in the order of vgicp_finalize_error_kernel -- and hands the sum and
    // the completion word to the host (the by-factor form of the linearise, gp_vgicp_stream.hpp); small single factors and batches alike
    double* partials = nullptr;
    GP_TRY(arm_factor_arrival(b, &ps, 1, done, &partials));  // one double per factor
    GP_TRY(launch_tiles<gp::MODE_ERR>(b, ps, partials));
    write_empty_factors(b, nullptr, done.seq);
    GP_TRY(wait_words(b, F, done.seq));
    const bool dropped = take_dropped_error_words(b);
    if (dropped || !words_arrived(b, (int)F, done.seq)) {  // the finalize kernel does this call's sums
      gp::DoneFlags again;
      GP_TRY(recover_arrival(b, true, &again));
      GP_TRY(gp::launch_finalize_error_table(b->stream, b->d_factors.as<gp::FactorDesc>(), (int)F, partials, static_cast<double*>(b->h_out_dev), again));
      GP_TRY(wait_words(b, F, again.seq));
    }
    b->factor_arrive_dirty = false;
    memcpy(out_host, b->h_out.ptr, sizeof(double) * F);
    return GP_OK;
  }
  GP_TRY(launch_error(b, ps, reinterpret_cast<double*>(b->h_out_dev), done));
  GP_TRY(wait_words(b, F, done.seq));
  memcpy(out_host, b->h_out.ptr, sizeof(double) * F);
  return GP_OK;
}

int gp_vgicp_batch_time_linearize(gp_vgicp_batch_t* b, const double* poses_host, int iters, float* ms_total, float* ms_main_kernel, float* ms_finalize_kernel) {
  if (!b || !poses_host || iters <= 0) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_time_linearize: bad arguments");
  if (table_is_stale(b)) GP_TRY(build_table(b));
  const size_t F = b->factors.size();
  if (F == 0) return GP_OK;
  // the device work of the SYNCHRONOUS call (gp_vgicp_batch_linearize), incl. its split finalize for a single large factor
  const int parts = (F == 1 && takes_rigid_path(b, poses_host) && b->num_tiles >= kFinalizeSplitTiles) ? kFinalizeParts : 1;
  gp::DeviceArray d_out;
  GP_TRY(d_out.alloc(sizeof(gp_linearized6) * F * (size_t)parts));
  PoseSource ps;
  GP_TRY(stage_poses(b, poses_host, nullptr, &ps));
  double* partials = nullptr;
  GP_TRY(partials_ptr(b, &partials));
  const bool rigid = takes_rigid_path(b, poses_host);
  hipEvent_t e0, e1, e2;
  GP_HIP(hipEventCreate(&e0));
  GP_HIP(hipEventCreate(&e1));
  GP_HIP(hipEventCreate(&e2));
  GP_TRY(launch_linearize(b, ps, d_out.as<gp_linearized6>(), rigid, {}, parts));  // warm-up
  GP_HIP(hipStreamSynchronize(b->stream));
  // whole pass, back to back
  GP_HIP(hipEventRecord(e0, b->stream));
  for (int i = 0; i < iters; i++) GP_TRY(launch_linearize(b, ps, d_out.as<gp_linearized6>(), rigid, {}, parts));
  GP_HIP(hipEventRecord(e1, b->stream));
  GP_HIP(hipEventSynchronize(e1));
  float t_total = 0.f;
  GP_HIP(hipEventElapsedTime(&t_total, e0, e1));
  // main kernel alone, then finalize alone (same stream the product path launches on)
  GP_HIP(hipEventRecord(e0, b->stream));
  for (int i = 0; i < iters; i++) GP_TRY(rigid ? launch_tiles<gp::MODE_LIN>(b, ps, partials) : launch_tiles<gp::MODE_LIN_GENERAL>(b, ps, partials));
  GP_HIP(hipEventRecord(e1, b->stream));
  for (int i = 0; i < iters; i++)
    GP_TRY(rigid ? launch_finalize<false>(b, ps, partials, d_out.as<gp_linearized6>(), {}, parts) : launch_finalize<true>(b, ps, partials, d_out.as<gp_linearized6>()));
  GP_HIP(hipEventRecord(e2, b->stream));
  GP_HIP(hipEventSynchronize(e2));
  float t_main = 0.f, t_fin = 0.f;
  GP_HIP(hipEventElapsedTime(&t_main, e0, e1));
  GP_HIP(hipEventElapsedTime(&t_fin, e1, e2));
  if (ms_total) *ms_total = t_total / (float)iters;
  if (ms_main_kernel) *ms_main_kernel = t_main / (float)iters;
  if (ms_finalize_kernel) *ms_finalize_kernel = t_fin / (float)iters;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipEventDestroy(e2);
  return GP_OK;
}

}  // extern "C"
