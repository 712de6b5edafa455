// gp_vgicp_table.hip -- what a VGICP batch knows before it launches: its tuning, the extents of its sources, the factor / tile table and when it is stale, which
// kernels a set of poses takes (takes_rigid_path) and how poses reach a launch (stage_poses); beside them the byte accounting of a built table and
// batch_set_sources_shared.  The entry points are gp_vgicp_batch.hip and gp_vgicp_debug.hip, the kernels and their launches gp_vgicp.hip; what they share is
// gp_vgicp_batch.hpp.
//
// Replaces (reference): the host side of src/gtsam_points/factors/integrated_vgicp_derivatives{,_linearize,_compute,_inliers}.cu.
#include <algorithm>
#include <cstring>

#include "gp_host.hpp"
#include "gp_vgicp_batch.hpp"

namespace {

constexpr int kPlanMinPoints = 65536;  // single factors below this keep the fixed tiles of a batch (their records then do not depend on how they are batched)

// ---- per-batch tuning (nothing process-global: SURVEY.md 8(b) "re-entrant across handles") --------------------------------------------------
// the keys that are one int of gp_vgicp_tuning.  lo > hi: a switch, stored as 0 / 1.  GP_TUNE_KERNEL (a set of values) and the XCD weights are apply_tuning's own.
struct TuneKey {
  int key;
  int gp_vgicp_tuning::*member;
  int lo, hi;
  bool readable;
  const char* range_error;
};
constexpr TuneKey kTuneKeys[] = {
    {GP_TUNE_SOURCE_POLICY, &gp_vgicp_tuning::source_policy, 0, 2, true, "GP_TUNE_SOURCE_POLICY: 0 (per batch), 1 (default cache policy), 2 (non-temporal)"},
    {GP_TUNE_XCD_CHUNK, &gp_vgicp_tuning::xcd_chunk, 0, 4096, true, "GP_TUNE_XCD_CHUNK: 0 (contiguous eighths) .. 4096 tiles per run"},
    {GP_TUNE_STAGGER, &gp_vgicp_tuning::stagger, 0, 64, true, "GP_TUNE_STAGGER: 0..64 (x 512 clocks)"},
    {GP_TUNE_TILE_INTERLEAVE, &gp_vgicp_tuning::tile_interleave, 1, 0, true, nullptr},
    {GP_TUNE_FUSED_FINALIZE, &gp_vgicp_tuning::fused_finalize, 1, 0, true, nullptr},
    {GP_TUNE_MAX_WORKGROUPS, &gp_vgicp_tuning::max_wgs, 8, 1024, false, "GP_TUNE_MAX_WORKGROUPS: 8 .. 1024"},
    {GP_TUNE_TILE_CHUNKS, &gp_vgicp_tuning::tile_chunks, 0, 64, true, "GP_TUNE_TILE_CHUNKS: 0 (automatic) .. 64 chunks per wave"},
    {GP_TUNE_SOURCE_MIRROR, &gp_vgicp_tuning::source_mirror, 1, 0, true, nullptr},
    {GP_TUNE_FAR_POSE_RATIO, &gp_vgicp_tuning::far_pose_ratio, 0, 1000000, true, "GP_TUNE_FAR_POSE_RATIO: 0 (no pose counts as far) .. 1000000 (x the source cloud's extent)"},
    // make_stream_plan refuses a skew that overdraws an XCD's share and deals that launch flat
    {GP_TUNE_BALANCE, &gp_vgicp_tuning::balance, -1, 1000, true, "GP_TUNE_BALANCE: -1 (automatic), 0 (flat) .. 1000 (per mille of the mean share per dispatch round)"},
};

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

// ---- the stages of build_table ------------------------------------------------------------------------------------------------------------------

// the factor descriptors, the family this batch really runs and the cache policy of its source stream
int resolve_family(gp_vgicp_batch* b, std::vector<gp::FactorDesc>* descs) {
  const int F = (int)b->factors.size();
  b->total_points = 0;
  b->use_grid = true;
  b->any_sv = false;
  // the hashed family reads the maps' private line tables, which a map with a block grid builds only now (gp_voxelmap::ensure_private_table)
  bool all_grid = true;
  for (const auto* f : b->factors) {
    if (!f->target->loaded()) return gp::fail(GP_ERROR_NOT_LOADED, "VGICP factor: target voxel map is not loaded on the GPU");
    if (!f->target->has_grid) all_grid = false;
  }
  if (!all_grid || b->tuning.kernel == GP_KERNEL_HASHED)
    for (const auto* f : b->factors) GP_TRY(const_cast<gp_voxelmap*>(f->target)->ensure_private_table());  // (a cache of the map, not its state)
  bool offsets32 = true;
  std::vector<const float*> srcs;
  for (int i = 0; i < F; i++) {
    const gp_vgicp_factor* f = b->factors[i];
    gp::FactorDesc& d = (*descs)[i];
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
    srcs.push_back(d.points);
  }
  int fam = b->tuning.kernel;
  if (fam == GP_KERNEL_STREAM && (!b->use_grid || !offsets32)) fam = GP_KERNEL_LOOKAHEAD;
  if ((fam == GP_KERNEL_LOOKAHEAD || fam == GP_KERNEL_GRID_F64) && !b->use_grid) fam = GP_KERNEL_HASHED;
  b->family = fam;
  std::sort(srcs.begin(), srcs.end());
  b->stream_once = b->shares_device_ok && std::adjacent_find(srcs.begin(), srcs.end()) == srcs.end();
  b->nt = b->tuning.source_policy == 2 || (b->tuning.source_policy == 0 && b->stream_once);
  return GP_OK;
}

// the packed source mirrors (gp::SourceMirror): built once per cloud, here, where a table upload synchronises anyway.  The batch streams them when
// EVERY factor with a full chunk has a usable one (a cloud with an unsymmetric covariance has none and keeps the whole batch on the caller's arrays)
int acquire_mirrors(gp_vgicp_batch* b, std::vector<gp::FactorDesc>* descs) {
  const int F = (int)b->factors.size();
  b->packed = false;
  if (b->family == GP_KERNEL_STREAM && b->tuning.source_mirror) {
    bool all = F > 0;
    for (int i = 0; i < F; i++) {
      gp_vgicp_factor* f = b->factors[i];
      if (!f->mirror_tried) {
        GP_TRY(gp::acquire_source_mirror(f->points, f->covs, f->n, f->device, b->stream, &f->mirror));
        f->mirror_tried = true;
      }
      if (f->mirror && f->mirror->usable) (*descs)[i].packed = f->mirror->data.as<char>();
      else if (f->n >= gp::kChunkPoints) all = false;
    }
    b->packed = all;
  }
  if (!b->packed)
    for (auto& d : *descs) d.packed = nullptr;
  return GP_OK;
}

// 64-point chunks per wave of a fixed tile (a tile = 256 x this many points): a function of the factors' sizes, the family and the tuning alone
int chunks_per_wave(const std::vector<gp::FactorDesc>& descs, int family, const gp_vgicp_tuning& tuning) {
  // the hashed-line-table, reference-shaped and f64 kernels exist for 1024-point tiles only (round 6: so does the LOOKAHEAD family -- it exists for maps of
  // >= 2^26 voxels, where no batch is small; its 512- / 256-point instantiations went with that: VERDICT r05 #8)
  if (family != GP_KERNEL_STREAM) return gp::kPipelineChunks;
  if (tuning.tile_chunks > 0) return tuning.tile_chunks;
  auto tiles_of = [&](int points) {
    int64_t count = 0;
    for (const auto& d : descs) count += (d.n + points - 1) / points;
    return count;
  };
  // the stream kernel takes tiles of any whole number of chunks.  4096-point tiles from 4096 such tiles up (a C4 shard: 512 factors x 8): with the factors finalized
  // inside the tile kernel every tile ends with a write-through row and an arrival, so fewer, larger tiles win while there are still four rounds of them (C4 shard
  // 0.171 -> 0.163 ms; C3, 1536 such tiles: no)
  if (tiles_of(4096) >= 4 * gp::kResidentWorkgroups) return 16;
  // 2048-point tiles (eight chunks per wave: the cold start of the pipeline is paid half as often) where that still leaves two rounds of workgroups -- C3 56.7 ->
  // 51.3 us, C4 shard 135 -> 115 us, whole C4 1.08 -> 1.00 ms (profiles/r03_tile_chunks.jsonl; 4096-point tiles: C3 54.7, C4 shard 114)
  if (tiles_of(2048) >= 2 * gp::kResidentWorkgroups) return 8;
  // else the largest tile that still fills 3/4 of the chip's resident workgroups, so that a 15 k-point scan is not left to 15 workgroups
  for (int cand : {4, 2})
    if (tiles_of(256 * cand) >= gp::kResidentWorkgroups * 3 / 4) return cand;
  return 1;
}

// the tile list: the balanced plan of one large factor of the stream family, else fixed tiles, factor after factor
void make_tiles(gp_vgicp_batch* b, std::vector<gp::FactorDesc>* descs, std::vector<gp::TileDesc>* tiles) {
  const int F = (int)descs->size();
  b->planned = b->family == GP_KERNEL_STREAM && F == 1 && (*descs)[0].n >= kPlanMinPoints;
  if (b->planned) {
    // the table holds the same tiles the in-argument launch derives from the plan (plan_tile)
    gp::FactorDesc& d = (*descs)[0];
    d.tile_count = gp::make_stream_plan(d.n, b->tuning.balance, b->tuning.xcd_weights_set ? b->tuning.xcd_weights : nullptr, &b->plan, b->tuning.max_wgs);
    d.tile_begin = 0;
    b->ppt = 4;
    b->tile_points = 0;
    gp::for_each_plan_tile(b->plan, [&](int t, int begin, int count) { tiles->push_back(gp::TileDesc{0, begin, count, t}); });
  } else {
    b->ppt = chunks_per_wave(*descs, b->family, b->tuning);
    b->tile_points = 64 * 4 * b->ppt;
    for (int i = 0; i < F; i++) {
      gp::FactorDesc& d = (*descs)[i];
      d.tile_begin = (int)tiles->size();
      for (int t = 0, T = gp::fixed_tile_count(d.n, b->tile_points); t < T; t++) {
        int begin = 0, count = 0;
        gp::fixed_tile(t, d.n, b->tile_points, &begin, &count);
        tiles->push_back(gp::TileDesc{i, begin, count, (int)tiles->size()});
      }
      d.tile_count = (int)tiles->size() - d.tile_begin;
    }
  }
  b->num_tiles = (int)tiles->size();
}

// execution order (GP_TUNE_TILE_INTERLEAVE): consecutive factors that read the SAME source cloud (a submap matched against several targets, BASELINE configs[3])
// take turns tile by tile, so the workgroups that run side by side on an XCD read the same source bytes at the same time -- one of them misses L2, the others
// hit.  Partial rows stay factor-major (TileDesc::row).
void interleave_tiles(const std::vector<gp::FactorDesc>& descs, std::vector<gp::TileDesc>* tiles) {
  const int F = (int)descs.size();
  std::vector<gp::TileDesc> order;
  order.reserve(tiles->size());
  for (int i = 0; i < F;) {
    int j = i + 1;
    while (j < F && descs[j].points == descs[i].points && descs[j].covs == descs[i].covs && descs[j].n == descs[i].n) j++;
    for (int t = 0; t < descs[i].tile_count; t++)
      for (int k = i; k < j; k++) order.push_back((*tiles)[(size_t)descs[k].tile_begin + t]);
    i = j;
  }
  tiles->swap(order);
}

// the batch's buffers at the table's sizes, and the two tables on the device
int upload_table(gp_vgicp_batch* b, const std::vector<gp::FactorDesc>& descs, const std::vector<gp::TileDesc>& tiles) {
  const size_t F = descs.size(), slots = std::max(F, (size_t)gp::kFinalizePartsMax);
  GP_TRY(b->d_factors.ensure(sizeof(gp::FactorDesc) * std::max<size_t>(F, 1)));
  GP_TRY(b->d_tiles.ensure(sizeof(gp::TileDesc) * (size_t)std::max(b->num_tiles, 1)));
  GP_TRY(b->d_poses.ensure(sizeof(double) * 32 * std::max<size_t>(F, 1)));
  GP_TRY(b->h_poses.ensure(sizeof(double) * 32 * std::max<size_t>(F, 1)));
  GP_TRY(b->h_out.ensure(sizeof(gp_linearized6) * slots));
  GP_HIP(hipHostGetDevicePointer(&b->h_out_dev, b->h_out.ptr, 0));
  gp::PinnedArray& h_done = b->arrival.h_done;
  const size_t before = h_done.bytes;
  GP_TRY(h_done.ensure(sizeof(unsigned long long) * slots));
  if (h_done.bytes != before) memset(h_done.ptr, 0, h_done.bytes);
  GP_HIP(hipHostGetDevicePointer(&b->arrival.h_done_dev, h_done.ptr, 0));
  if (!b->temp_buffer) GP_TRY(b->d_partials.ensure(sizeof(double) * gp::ACCG_STRIDE * (size_t)std::max(b->num_tiles, 1)));
  // the table upload is synchronous (pageable source); it happens once per factor-set change, not per linearise
  if (F) GP_HIP(hipMemcpy(b->d_factors.ptr, descs.data(), sizeof(gp::FactorDesc) * F, hipMemcpyHostToDevice));
  if (b->num_tiles) GP_HIP(hipMemcpy(b->d_tiles.ptr, tiles.data(), sizeof(gp::TileDesc) * (size_t)b->num_tiles, hipMemcpyHostToDevice));
  return GP_OK;
}

// is the 3x3 block of every pose orthonormal to 1e-9?  (gp::pose_is_rigid, gp_vgicp_shared.hpp)
bool poses_are_rigid(const double* poses_host, size_t F) {
  if (!poses_host) return false;
  for (size_t i = 0; i < F; i++)
    if (!gp::pose_is_rigid(poses_host + 16 * i)) return false;
  return true;
}

}  // namespace

namespace gp {

int apply_tuning(gp_vgicp_tuning* t, int key, int value) {
  if (key == GP_TUNE_KERNEL) {
    if (value != GP_KERNEL_REFERENCE && value != GP_KERNEL_HASHED && value != GP_KERNEL_GRID_F64 && value != GP_KERNEL_LOOKAHEAD && value != GP_KERNEL_STREAM)
      return gp::fail(GP_ERROR_INVALID_ARGUMENT, "GP_TUNE_KERNEL: one of GP_KERNEL_REFERENCE (0), _HASHED (2), _GRID_F64 (3), _LOOKAHEAD (8), _STREAM (12)");
    t->kernel = value;
    return GP_OK;
  }
  if (key >= GP_TUNE_XCD_WEIGHT_0 && key < GP_TUNE_XCD_WEIGHT_0 + 8) {
    if (value < 500 || value > 1500) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "GP_TUNE_XCD_WEIGHT_x: 500..1500 (per mille of the mean share)");
    t->xcd_weights[key - GP_TUNE_XCD_WEIGHT_0] = value;
    t->xcd_weights_set = true;
    return GP_OK;
  }
  for (const TuneKey& k : kTuneKeys)
    if (k.key == key) {
      if (k.lo > k.hi) value = value ? 1 : 0;
      else if (value < k.lo || value > k.hi) return gp::fail(GP_ERROR_INVALID_ARGUMENT, k.range_error);
      t->*k.member = value;
      return GP_OK;
    }
  return gp::fail(GP_ERROR_INVALID_ARGUMENT, "unknown GP_TUNE_* key");
}

bool read_tuning(const gp_vgicp_tuning& t, int key, int* value) {
  if (key == GP_TUNE_KERNEL) {
    *value = t.kernel;
    return true;
  }
  for (const TuneKey& k : kTuneKeys)
    if (k.key == key && k.readable) {
      *value = t.*k.member;
      return true;
    }
  return false;
}

int build_table(gp_vgicp_batch* b) {
  const size_t F = b->factors.size();
  std::vector<gp::FactorDesc> descs(F);
  std::vector<gp::TileDesc> tiles;
  GP_TRY(resolve_family(b, &descs));
  GP_TRY(acquire_mirrors(b, &descs));
  make_tiles(b, &descs, &tiles);
  if (b->tuning.tile_interleave && !b->planned) interleave_tiles(descs, &tiles);
  b->h_descs = descs;
  GP_TRY(upload_table(b, descs, tiles));
  GP_TRY(measure_extents(b));
  b->seen.resize(F);
  for (size_t i = 0; i < F; i++) b->seen[i] = b->factors[i]->generation + b->factors[i]->target->generation;
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
  return ensure_table(f->self_batch);
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

// poses for a launch: a single factor carries them in the kernel arguments; a batch uploads them with one H2D
// zero_copy (the SYNCHRONOUS entry points, which return only after the kernels have finished): the kernels read the poses straight
// out of the pinned staging buffer over the fabric -- one 128-B scalar read per workgroup, hidden behind the other workgroups -- instead
// of behind a copy-engine transfer (an API call, an event and ~10 us of SDMA start-up in front of the first kernel).  The asynchronous
// issue_* entry points keep the H2D copy: the caller may re-stage poses while the kernels of the previous pass are still running.
int stage_poses(gp_vgicp_batch* b, const double* lin, const double* eval, PoseSource* ps, bool zero_copy) {
  const size_t F = b->factors.size();
  if (F == 1) {
    inline_poses(b, lin, eval, ps);
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
  const double* tables = b->d_poses.as<double>();
  if (zero_copy) {
    void* hd = nullptr;
    GP_HIP(hipHostGetDevicePointer(&hd, h, 0));
    tables = static_cast<const double*>(hd);
  } else {
    GP_HIP(hipMemcpyAsync(b->d_poses.ptr, h, sizeof(double) * 16 * F * (eval ? 2 : 1), hipMemcpyHostToDevice, b->stream));
    GP_HIP(hipEventRecord(b->h2d_done, b->stream));
  }
  ps->d_lin = tables;
  ps->d_eval = eval ? tables + 16 * F : nullptr;
  ps->inl.use = 0;
  return GP_OK;
}

// gp_multi.hip: several shards of one multi-batch run on this device and read the same source clouds one after the other, so the source
// stream of this batch must stay cacheable (no non-temporal policy)
void batch_set_sources_shared(gp_vgicp_batch* batch, bool shared) {
  if (!batch || batch->shares_device_ok == !shared) return;
  batch->shares_device_ok = !shared;
  batch->table_dirty = true;
}

}  // namespace gp

extern "C" {

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
  if (!batch || gp::ensure_table(batch) != GP_OK) return 0;
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

}  // extern "C"
