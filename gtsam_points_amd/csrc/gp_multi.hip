// gp_multi.hip -- many-factor VGICP batches sharded over the GPUs of one node, driven from ONE process.
//
// The reference has no multi-GPU code: NonlinearFactorSetGPU::linearize (src/gtsam_points/cuda/nonlinear_factor_set_gpu.cpp:64-139)
// walks its factors on one device.  Factors are independent units (one source cloud, one target map, one pose pair in, one
// 122-scalar record out), so the factor list is partitioned into shards, every shard runs the batched kernels of gp_vgicp.hip on
// its own device and stream, and the one exchange step is the all-reduce BASELINE.json's north_star names:
//
//     every shard writes its records into its rows of a zeroed [F x 122] f64 stack on its device
//     ONE ncclAllReduce(sum) per device over that stack (RCCL over xGMI; every row has exactly one writer, so the sum is exact)
//     ONE D2H of the complete stack from the first shard's device
//
// Round 4: the stack has one writer per row and gp_shard_plan deals contiguous ranges, so when the shards are EQUAL contiguous ranges in rank order (C4: 8 x 512
// factors) the same exchange is an in-place ncclAllGather -- (N-1)/N of the stack per device instead of 2 (N-1)/N, and no zeroing ("the equivalent
// cheaper form").  use_rccl = 2 asks for it (falls back to the all-reduce when the plan does not qualify); gp_vgicp_multi_batch_uses_rccl tells which runs.
//
// RCCL is loaded with dlopen when a multi-batch really spans several devices (gp_rccl.hpp).  Where it is not used -- all shards on one device (the single-GPU
// rehearsal of an N-shard plan), a missing library, or use_rccl == 0 -- NO collective and no copy runs at all: every shard's finalize kernel stores its records
// straight into its rows of ONE host-pinned, portable stack (the consumer is host-side), and the pass ends with the shards' streams' synchronisation.
//
// Which factors a shard holds and where their rows lie is gp_shard_layout.hpp's (host arithmetic, with the balanced plan behind gp_shard_plan_*).  Everything here is
// built on the public per-device entry points (gp_vgicp_batch_*), one host thread issuing to all devices.
#include <algorithm>
#include <cstring>
#include <deque>
#include <memory>
#include <string>

#include "gp_host.hpp"
#include "gp_rccl.hpp"
#include "gp_shard_layout.hpp"

namespace {

// out[index[f]][c] = local[f][c]: a shard whose factors are not one contiguous range of the global list
__global__ void __launch_bounds__(256) scatter_rows_kernel(const double* __restrict__ local, const int* __restrict__ index, double* __restrict__ stack, int n, int width) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n * width) return;
  const int f = t / width, c = t % width;
  stack[(size_t)index[f] * width + c] = local[(size_t)f * width + c];
}

constexpr int kRecordDoubles = (int)(sizeof(gp_linearized6) / sizeof(double));  // 122

struct DeviceGuard {
  int saved = 0;
  DeviceGuard() { (void)hipGetDevice(&saved); }
  ~DeviceGuard() { (void)hipSetDevice(saved); }
};

struct Shard {
  int device = -1;
  hipStream_t stream = nullptr;
  gp_vgicp_batch_t* batch = nullptr;
  gp::ShardRows rows;  // which factors of the global list, and whether they are one range of it
  int64_t points = 0;
  gp::DeviceArray d_stack;   // [F_total x 122] f64 (RCCL) or [F_local x 122] (host gather)
  gp::DeviceArray d_err;     // [F_total] / [F_local] f64
  gp::DeviceArray d_index;   // int[F_local] when !contiguous
  gp::DeviceArray d_local;   // [F_local x 122] staging when !contiguous under RCCL
  std::vector<double> poses, poses_eval;
  hipEvent_t e_begin = nullptr, e_compute = nullptr, e_done = nullptr;
  ncclComm_t comm = nullptr;
  ~Shard() {  // on its device, the stream drained first (the batch's destructor restores the caller's device)
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (comm && rccl().ok) (void)rccl().CommDestroy(comm);
    if (batch) gp_vgicp_batch_destroy(batch);
    d_stack.release();
    d_err.release();
    d_index.release();
    d_local.release();
    if (e_begin) (void)hipEventDestroy(e_begin);
    if (e_compute) (void)hipEventDestroy(e_compute);
    if (e_done) (void)hipEventDestroy(e_done);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

}  // namespace

struct gp_shard_plan {
  std::vector<int> begin;  // num_shards + 1 boundaries
};

struct gp_vgicp_multi_batch {
  std::deque<Shard> shards;  // (a Shard owns device arrays: it never moves)
  int num_factors = 0;
  bool use_rccl = false;
  bool gather = false;      // the exchange is an in-place ncclAllGather (equal contiguous shards in rank order) instead of the all-reduce
  size_t gather_rows = 0;   // ... rows per shard
  gp::PinnedArray h_stack;  // [F_total x 122] f64, pinned + portable: results land here (written by the finalize kernels themselves when no collective runs)
  gp::PinnedArray h_err;    // [F_total] f64, likewise
  float last_ms_compute = 0.f, last_ms_exchange = 0.f;
  ~gp_vgicp_multi_batch() {  // the shards in order, then the host stacks
    DeviceGuard guard;
    while (!shards.empty()) shards.pop_front();
    h_stack.release();
    h_err.release();
  }
};

namespace {

// one pass over all shards: `width` doubles per factor (122: linearise, 1: error) into the host stack `host`, through the shard's array `array`
struct Pass {
  int width;
  double* host;
  gp::DeviceArray Shard::*array;
};

// where issue() writes for this shard and pass, and whether scatter_rows_kernel follows
struct Destination {
  double* ptr = nullptr;
  bool scatter = false;
};

int destination_of(const gp_vgicp_multi_batch* mb, Shard& s, const Pass& p, Destination* out) {
  double* mine = (s.*p.array).as<double>();
  const size_t first = (size_t)s.rows.first_row * p.width;
  if (mb->use_rccl && s.rows.contiguous) {  // collective, contiguous: its own rows of the device stack
    *out = {mine + first, false};
  } else if (mb->use_rccl) {  // collective, non-contiguous: local staging, scattered into the device stack
    *out = {s.d_local.as<double>(), true};
  } else if (s.rows.contiguous) {
    // no collective, contiguous: the finalize kernel's record stores go straight into the shard's rows of the host stack (pinned, portable: every device sees it
    // at the same address): no device-side stack, no copy operation, nothing left to do but wait for the streams
    void* hd = nullptr;
    GP_HIP(hipHostGetDevicePointer(&hd, p.host + first, 0));
    *out = {static_cast<double*>(hd), false};
  } else {  // no collective, non-contiguous: local rows, copied out one by one after the compute
    *out = {mine, false};
  }
  return GP_OK;
}

template <typename Issue>
int run_pass_impl(gp_vgicp_multi_batch* mb, const Pass& p, Issue issue, double* out_host, bool* group_open) {
  DeviceGuard guard;
  const int width = p.width;
  const size_t F = (size_t)mb->num_factors;
  double* h = p.host;
  // ---- compute: every shard issues its batched kernels into its rows ----
  const bool zero = mb->use_rccl && !mb->gather;  // (the all-gather overwrites every row; the all-reduce adds zeros to all rows but the writer's)
  for (auto& s : mb->shards) {
    GP_HIP(hipSetDevice(s.device));
    gp::DeviceArray& dst = s.*p.array;
    GP_HIP(hipEventRecord(s.e_begin, s.stream));
    if (zero) GP_HIP(hipMemsetAsync(dst.ptr, 0, sizeof(double) * width * F, s.stream));
    if (!s.rows.index.empty()) {
      Destination to;
      GP_TRY(destination_of(mb, s, p, &to));
      GP_TRY(issue(s, to.ptr));
      if (to.scatter) {
        const int n = (int)s.rows.index.size();
        hipLaunchKernelGGL(scatter_rows_kernel, dim3((n * width + 255) / 256), dim3(256), 0, s.stream, (const double*)s.d_local.as<double>(),
                           (const int*)s.d_index.as<int>(), dst.as<double>(), n, width);
        GP_HIP(hipGetLastError());
      }
    }
    GP_HIP(hipEventRecord(s.e_compute, s.stream));
  }
  // ---- exchange ----
  if (mb->use_rccl) {
    Rccl& r = rccl();
    GP_NCCL(r.GroupStart());
    *group_open = true;
    for (auto& s : mb->shards) {
      gp::DeviceArray& dst = s.*p.array;
      if (mb->gather) {
        const size_t count = mb->gather_rows * (size_t)width;  // in place: rank k's send buffer is its own slot of the receive buffer
        GP_NCCL(r.AllGather(dst.as<double>() + gp::gather_send_offset(s.rows, width), dst.ptr, count, ncclDouble, s.comm, s.stream));
      } else {
        GP_NCCL(r.AllReduce(dst.ptr, dst.ptr, (size_t)width * F, ncclDouble, ncclSum, s.comm, s.stream));
      }
    }
    *group_open = false;
    GP_NCCL(r.GroupEnd());
    Shard& s0 = mb->shards[0];
    GP_HIP(hipSetDevice(s0.device));
    GP_HIP(hipMemcpyAsync(h, (s0.*p.array).ptr, sizeof(double) * width * F, hipMemcpyDeviceToHost, s0.stream));
    for (auto& s : mb->shards) {
      GP_HIP(hipSetDevice(s.device));
      GP_HIP(hipEventRecord(s.e_done, s.stream));
    }
  } else {
    for (auto& s : mb->shards) {
      GP_HIP(hipSetDevice(s.device));
      if (!s.rows.index.empty() && !s.rows.contiguous) {
        const double* src = (s.*p.array).as<double>();
        for (size_t k = 0; k < s.rows.index.size(); k++)
          GP_HIP(hipMemcpyAsync(h + (size_t)s.rows.index[k] * width, src + k * width, sizeof(double) * width, hipMemcpyDeviceToHost, s.stream));
      }
      GP_HIP(hipEventRecord(s.e_done, s.stream));
    }
  }
  float ms_compute = 0.f, ms_total = 0.f;
  for (auto& s : mb->shards) {
    GP_HIP(hipSetDevice(s.device));
    GP_HIP(hipEventSynchronize(s.e_done));
    float a = 0.f, b = 0.f;
    GP_HIP(hipEventElapsedTime(&a, s.e_begin, s.e_compute));
    GP_HIP(hipEventElapsedTime(&b, s.e_begin, s.e_done));
    ms_compute = std::max(ms_compute, a);
    ms_total = std::max(ms_total, b);
  }
  mb->last_ms_compute = ms_compute;
  mb->last_ms_exchange = std::max(0.f, ms_total - ms_compute);
  memcpy(out_host, h, sizeof(double) * width * F);
  return GP_OK;
}

// A failure in the middle of a pass must not leave an RCCL group open or work in flight on the other devices' streams (the next collective of
// this thread would hang or misbehave): the group is closed and every shard's stream drained before the error is handed up.
template <typename Issue>
int run_pass(gp_vgicp_multi_batch* mb, const Pass& p, Issue issue, double* out_host) {
  bool group_open = false;
  const int rc = run_pass_impl(mb, p, issue, out_host, &group_open);
  if (rc != GP_OK) {
    const std::string keep = gp_last_error() ? gp_last_error() : "";
    if (group_open) (void)rccl().GroupEnd();
    for (auto& s : mb->shards) {
      (void)hipSetDevice(s.device);
      if (s.stream) (void)hipStreamSynchronize(s.stream);
    }
    (void)hipGetLastError();
    gp::fail(rc, keep.c_str());  // (the clean-up calls may have replaced the message)
  }
  return rc;
}

// every shard's rows of the caller's [F x 16] poses, packed into the shard's own array
void stage_poses(gp_vgicp_multi_batch* mb, const double* poses_host, std::vector<double> Shard::*to) {
  for (auto& s : mb->shards)
    for (size_t k = 0; k < s.rows.index.size(); k++) memcpy((s.*to).data() + 16 * k, poses_host + 16 * (size_t)s.rows.index[k], sizeof(double) * 16);
}

// the shard's resources on its device: stream, batch over its factors, arrays, events
int open_shard(Shard& s, gp_vgicp_factor_t* const* factors, size_t F, bool use_rccl, bool shares_device) {
  if (hipSetDevice(s.device) != hipSuccess || hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess)
    return gp::fail(GP_ERROR_HIP, "gp_vgicp_multi_batch_create: cannot create a stream on the shard's device");
  const std::vector<int>& index = s.rows.index;
  std::vector<gp_vgicp_factor_t*> mine;
  for (int i : index) mine.push_back(factors[i]);
  GP_TRY(gp_vgicp_batch_create(mine.data(), (int)mine.size(), s.stream, &s.batch));
  if (shares_device) gp::batch_set_sources_shared(s.batch, true);  // sibling shards on this device re-read the clouds: keep the stream cacheable
  const size_t rows = use_rccl ? std::max<size_t>(F, 1) : std::max<size_t>(index.size(), 1);
  GP_TRY(s.d_stack.alloc(sizeof(double) * kRecordDoubles * rows));
  GP_TRY(s.d_err.alloc(sizeof(double) * rows));
  if (use_rccl && !s.rows.contiguous) {
    GP_TRY(s.d_local.alloc(sizeof(double) * kRecordDoubles * index.size()));
    GP_TRY(s.d_index.alloc(sizeof(int) * index.size()));
    if (hipMemcpy(s.d_index.ptr, index.data(), sizeof(int) * index.size(), hipMemcpyHostToDevice) != hipSuccess)
      return gp::fail(GP_ERROR_HIP, "gp_vgicp_multi_batch_create: index upload failed");
  }
  s.poses.resize(16 * index.size());
  s.poses_eval.resize(16 * index.size());
  if (hipEventCreate(&s.e_begin) != hipSuccess || hipEventCreate(&s.e_compute) != hipSuccess || hipEventCreate(&s.e_done) != hipSuccess)
    return gp::fail(GP_ERROR_HIP, "gp_vgicp_multi_batch_create: hipEventCreate failed");
  return GP_OK;
}

}  // namespace

extern "C" {

int gp_shard_plan_create(const int64_t* weights, int num_factors, int num_shards, gp_shard_plan_t** out) {
  if (!out || num_factors < 0 || num_shards <= 0 || (num_factors > 0 && !weights)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_shard_plan_create: bad arguments");
  for (int i = 0; i < num_factors; i++)
    if (weights[i] < 0) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_shard_plan_create: negative weight");
  auto* p = new gp_shard_plan;
  p->begin = gp::balanced_boundaries(weights, num_factors, num_shards);
  *out = p;
  return GP_OK;
}

int gp_shard_plan_num_shards(const gp_shard_plan_t* plan) { return plan ? (int)plan->begin.size() - 1 : 0; }

int gp_shard_plan_range(const gp_shard_plan_t* plan, int shard, int* begin, int* end) {
  if (!plan || shard < 0 || shard + 1 >= (int)plan->begin.size() || !begin || !end) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_shard_plan_range: bad arguments");
  *begin = plan->begin[(size_t)shard];
  *end = plan->begin[(size_t)shard + 1];
  return GP_OK;
}

int gp_shard_plan_destroy(gp_shard_plan_t* plan) {
  delete plan;
  return GP_OK;
}

int gp_vgicp_multi_batch_create(gp_vgicp_factor_t* const* factors, int num_factors, const int* shard_of_factor, int num_shards, int use_rccl,
                                gp_vgicp_multi_batch_t** out) {
  if (!out || num_factors < 0 || (num_factors > 0 && !factors)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_multi_batch_create: bad arguments");
  DeviceGuard guard;
  // ---- shards: given explicitly, or one per device the factors live on (ascending device id) ----
  std::vector<int> by_device;
  if (shard_of_factor) {
    if (num_shards <= 0) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_multi_batch_create: num_shards must be positive with an explicit assignment");
  } else {
    std::vector<int> devs;
    for (int i = 0; i < num_factors; i++) devs.push_back(gp_vgicp_factor_device(factors[i]));
    std::vector<int> uniq = devs;
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    num_shards = std::max<int>(1, (int)uniq.size());
    for (int dev : devs) by_device.push_back((int)(std::lower_bound(uniq.begin(), uniq.end(), dev) - uniq.begin()));
    shard_of_factor = by_device.data();
  }
  gp::ShardLayout layout;
  const char* reason = "";
  if (gp::shard_layout(shard_of_factor, num_factors, num_shards, &layout, &reason) != GP_OK)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, std::string("gp_vgicp_multi_batch_create: ") + reason);
  std::unique_ptr<gp_vgicp_multi_batch> mb(new gp_vgicp_multi_batch);  // (whatever it holds when a stage below returns early goes with it)
  mb->num_factors = num_factors;
  mb->shards.resize((size_t)num_shards);
  for (int k = 0; k < num_shards; k++) mb->shards[(size_t)k].rows = std::move(layout.shards[(size_t)k]);
  int current = 0;
  (void)hipGetDevice(&current);
  for (int i = 0; i < num_factors; i++) {
    if (!factors[i]) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_multi_batch_create: null factor");
    Shard& s = mb->shards[(size_t)shard_of_factor[i]];
    const int dev = gp_vgicp_factor_device(factors[i]);
    if (s.device < 0) s.device = dev;
    if (s.device != dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_multi_batch_create: the factors of one shard live on different devices");
    s.points += gp_vgicp_factor_num_points(factors[i]);
  }
  for (auto& s : mb->shards)
    if (s.device < 0) s.device = current;  // an empty shard still takes part in the collective
  // ---- exchange mode: RCCL needs distinct devices (one rank per device in a communicator) ----
  std::vector<int> devlist;
  for (auto& s : mb->shards) devlist.push_back(s.device);
  std::vector<int> uniq = devlist;
  std::sort(uniq.begin(), uniq.end());
  const bool distinct = std::unique(uniq.begin(), uniq.end()) == uniq.end();
  // use_rccl: 0 = no collective (records straight into the host stack), 1 = ncclAllReduce of the zeroed stack, 2 = in-place ncclAllGather when the shards are equal
  // contiguous ranges in rank order (else the all-reduce), < 0 = automatic (2 when the batch spans several devices)
  bool want_rccl = use_rccl > 0 || (use_rccl < 0 && num_shards > 1);
  const bool want_gather = use_rccl == 2 || use_rccl < 0;
  if (want_rccl && (!distinct || !rccl().ok)) {
    if (use_rccl > 0)
      return gp::fail(GP_ERROR_INVALID_ARGUMENT, distinct ? "gp_vgicp_multi_batch_create: librccl.so could not be loaded" : "gp_vgicp_multi_batch_create: RCCL needs one shard per device");
    want_rccl = false;
  }
  mb->use_rccl = want_rccl;
  // ---- per-shard resources on the shard's device ----
  const size_t F = (size_t)num_factors;
  for (auto& s : mb->shards) GP_TRY(open_shard(s, factors, F, mb->use_rccl, !distinct));
  // portable: one address every device can store to (the no-collective pass) and the copy engine can write (the collective passes)
  const unsigned portable = hipHostMallocPortable | hipHostMallocMapped;
  if (mb->h_stack.ensure(sizeof(double) * kRecordDoubles * std::max<size_t>(F, 1), portable) != GP_OK || mb->h_err.ensure(sizeof(double) * std::max<size_t>(F, 1), portable) != GP_OK)
    return gp::fail(GP_ERROR_HIP, "gp_vgicp_multi_batch_create: hipHostMalloc (portable) failed");
  if (mb->use_rccl && want_gather) {
    mb->gather_rows = layout.gather_rows;
    mb->gather = mb->gather_rows > 0;
  }
  if (mb->use_rccl) {
    std::vector<ncclComm_t> comms((size_t)num_shards, nullptr);
    const ncclResult_t e = rccl().CommInitAll(comms.data(), num_shards, devlist.data());
    if (e != ncclSuccess) return nccl_fail(e, "ncclCommInitAll");
    for (int k = 0; k < num_shards; k++) mb->shards[(size_t)k].comm = comms[(size_t)k];
  }
  *out = mb.release();
  return GP_OK;
}

// Host only (no device is touched): what the in-place all-gather of a pass would send from, per shard, for this assignment -- the functions the pass itself
// uses. rows_per_shard = 0: the plan does not allow the all-gather (the pass would all-reduce).
int gp_debug_multi_gather_plan(const int* shard_of_factor, int num_factors, int num_shards, int width, int64_t* rows_per_shard, int64_t* send_offset_doubles) {
  if (!shard_of_factor || num_factors < 0 || num_shards <= 0 || width <= 0 || !rows_per_shard || !send_offset_doubles)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_debug_multi_gather_plan: bad arguments");
  gp::ShardLayout layout;
  const char* reason = "";
  if (gp::shard_layout(shard_of_factor, num_factors, num_shards, &layout, &reason) != GP_OK)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, std::string("gp_debug_multi_gather_plan: ") + reason);
  *rows_per_shard = (int64_t)layout.gather_rows;
  for (int k = 0; k < num_shards; k++) send_offset_doubles[k] = (int64_t)gp::gather_send_offset(layout.shards[(size_t)k], width);
  return GP_OK;
}

int gp_vgicp_multi_batch_destroy(gp_vgicp_multi_batch_t* batch) {
  delete batch;  // (its destructor and its shards' release everything, under a DeviceGuard)
  return GP_OK;
}

int gp_vgicp_multi_batch_size(const gp_vgicp_multi_batch_t* mb) { return mb ? mb->num_factors : 0; }
int gp_vgicp_multi_batch_num_shards(const gp_vgicp_multi_batch_t* mb) { return mb ? (int)mb->shards.size() : 0; }
int gp_vgicp_multi_batch_uses_rccl(const gp_vgicp_multi_batch_t* mb) { return mb && mb->use_rccl ? (mb->gather ? 2 : 1) : 0; }  // 0 no collective, 1 all-reduce, 2 all-gather

int gp_vgicp_multi_batch_shard_info(const gp_vgicp_multi_batch_t* mb, int shard, int* device, int* num_factors, int64_t* num_points) {
  if (!mb || shard < 0 || shard >= (int)mb->shards.size()) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_multi_batch_shard_info: bad arguments");
  const Shard& s = mb->shards[(size_t)shard];
  if (device) *device = s.device;
  if (num_factors) *num_factors = (int)s.rows.index.size();
  if (num_points) *num_points = s.points;
  return GP_OK;
}

int gp_vgicp_multi_batch_last_timing(const gp_vgicp_multi_batch_t* mb, float* ms_compute, float* ms_exchange) {
  if (!mb) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_multi_batch_last_timing: null");
  if (ms_compute) *ms_compute = mb->last_ms_compute;
  if (ms_exchange) *ms_exchange = mb->last_ms_exchange;
  return GP_OK;
}

int gp_vgicp_multi_batch_linearize(gp_vgicp_multi_batch_t* mb, const double* poses_host, gp_linearized6* out_host) {
  if (!mb || !poses_host || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_multi_batch_linearize: null");
  if (mb->num_factors == 0) return GP_OK;
  stage_poses(mb, poses_host, &Shard::poses);
  return run_pass(
    mb, Pass{kRecordDoubles, mb->h_stack.as<double>(), &Shard::d_stack},
    [](Shard& s, double* dst) { return gp_vgicp_batch_issue_linearize(s.batch, s.poses.data(), reinterpret_cast<gp_linearized6*>(dst)); }, reinterpret_cast<double*>(out_host));
}

int gp_vgicp_multi_batch_compute_error(gp_vgicp_multi_batch_t* mb, const double* poses_lin_host, const double* poses_eval_host, double* out_host) {
  if (!mb || !poses_lin_host || !poses_eval_host || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_multi_batch_compute_error: null");
  if (mb->num_factors == 0) return GP_OK;
  stage_poses(mb, poses_lin_host, &Shard::poses);
  stage_poses(mb, poses_eval_host, &Shard::poses_eval);
  return run_pass(
    mb, Pass{1, mb->h_err.as<double>(), &Shard::d_err}, [](Shard& s, double* dst) { return gp_vgicp_batch_issue_compute_error(s.batch, s.poses.data(), s.poses_eval.data(), dst); },
    out_host);
}

}  // extern "C"
