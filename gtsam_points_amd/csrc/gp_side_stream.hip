// gp_side_stream.hip -- the side stream of gp_estimate_covariances: a low-priority stream whose hardware queue does NOT share a dispatch pipe of the command processor
// with the caller's, picked once per host thread and device by a probe (pipe_probe_hog_kernel, pipe_probe_stamp_kernel).  gp_covariance.hip asks side_stream_for()
// for the handles; gp_trim_device_cache releases them (release_side_streams); gp_debug_side_stream_probe reports the probe's figures.
//
// Replaces: nothing upstream -- the reference estimates covariances on the CPU (features/covariance_estimation.cpp).
#include <algorithm>

#include "gp_host.hpp"

namespace gp {
// ---- the side stream of gp_estimate_covariances: a hardware queue that does NOT share a dispatch pipe with the caller's ----
// Two kernels on two HIP streams overlap only when their hardware queues sit on different pipes of the command processor: a pipe dispatches ONE grid at a time, and a
// grid with more workgroups than the device holds keeps its pipe until its last workgroup has been placed.  Measured (profiles/r05_c5_queue_pipes.txt): with the
// caller on queue 1 and the side stream on queue 3 the second covariance launch starts 8 us after the first; on queue 5 (the same process after bench.py's C4 phase had
// taken queues 2-4) it starts when the first launch's last workgroup is placed, 100 / 160 us later on the two 1 M-point clouds -- 0.07 ms per call.  HIP does not say
// which queue a stream gets, so the library asks the device: up to four low-priority streams are created (each gets a queue of its own from the runtime's pool for that
// priority), and the candidates are probed ONCE per host thread and device, beside the first caller stream that thread brings -- a grid of 6144 workgroups that holds two
// LDS-bound workgroups per CU for ~5 us each on the caller's stream, and one wave on the candidate that reports how long after the grid's first workgroup it got to run
// (~1 us on another pipe, the grid's whole dispatch on the same one).  The candidate with the shortest delay serves the thread's calls on that device from then on
// (~0.4 ms once).  Round 5 probed per caller stream (a 16-entry table keyed on the raw handle): an application that cycles streams re-paid 0.4 ms per new handle to save
// 0.07 ms per call, and a recycled handle inherited a stale choice -- a later caller stream on another pipe now simply keeps the first choice (correct either
// way: the choice only decides whether the two launches overlap).  gp_trim_device_cache() releases the thread's candidate streams, events and probe words.
// (extern "C": the two probe kernels keep their unmangled names, which the readers of the kernel traces know)
extern "C" __global__ void __launch_bounds__(256) pipe_probe_hog_kernel(unsigned long long* __restrict__ words, int ticks) {
  __shared__ float pad[12 * 1024];  // 48 KB: three workgroups per CU (160 KB of LDS), the wave slots stay free for the probe's wave
  pad[threadIdx.x * 48] = (float)threadIdx.x;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(words, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)ticks) __builtin_amdgcn_s_sleep(8);
  if (pad[(threadIdx.x * 48 + 7) % (12 * 1024)] < -1.0f) words[2] = 1;  // (keeps the array)
}
extern "C" __global__ void __launch_bounds__(64) pipe_probe_stamp_kernel(unsigned long long* __restrict__ words) {
  if (threadIdx.x != 0) return;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long seen = 0;
  while ((seen = __hip_atomic_load(words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0 && __builtin_amdgcn_s_memrealtime() - t0 < 200000ull) __builtin_amdgcn_s_sleep(4);  // (<= 2 ms)
  words[1] = __builtin_amdgcn_s_memrealtime();
}

struct SideStream {
  static constexpr int kCandidates = 4;
  struct PerDevice {
    SideStreamHandles cand[kCandidates];
    int num = 0;
    unsigned long long* words = nullptr;  // device: [0] first workgroup of the hog started, [1] the probe's wave ran, [2] unused
    struct Choice {
      hipStream_t caller;
      int index;
      float delay_us[kCandidates];
    } chosen{nullptr, 0, {-1.f, -1.f, -1.f, -1.f}};
    bool probed = false;
    bool created = false;
  };
  // releases what this thread holds for the current device (gp_trim_device_cache): the next covariance call creates and probes again
  static void release() {
    PerDevice* c = device_state();
    if (!c || !c->created) return;
    for (int i = 0; i < c->num; i++) {
      if (c->cand[i].stream) (void)hipStreamSynchronize(c->cand[i].stream), (void)hipStreamDestroy(c->cand[i].stream);
      if (c->cand[i].fork) (void)hipEventDestroy(c->cand[i].fork);
      if (c->cand[i].join) (void)hipEventDestroy(c->cand[i].join);
    }
    if (c->words) (void)hipFree(c->words);
    (void)hipGetLastError();
    *c = PerDevice{};
  }
  static PerDevice* device_state() {
    static thread_local PerDevice cache[16];
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 16) return nullptr;
    return &cache[d];
  }
  static void create(PerDevice& c) {
    c.created = true;
    // the LOWEST priority the device offers: what runs on the side stream fills the slots the caller's stream leaves free, it does not compete for them
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0, (void)hipGetLastError();
    for (int i = 0; i < kCandidates; i++) {
      SideStreamHandles n;
      if (hipStreamCreateWithPriority(&n.stream, hipStreamNonBlocking, least) != hipSuccess || hipEventCreateWithFlags(&n.fork, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&n.join, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        break;
      }
      c.cand[c.num++] = n;
    }
    if (c.num > 1 && hipMalloc(&c.words, 4 * sizeof(unsigned long long)) != hipSuccess) (void)hipGetLastError(), c.words = nullptr;
  }
  // delay (us) between the first workgroup of a pipe-filling grid on `caller` and a wave on the candidate; < 0: the probe did not run
  static float probe(PerDevice& c, hipStream_t caller, const SideStreamHandles& n) {
    unsigned long long h[2] = {0, 0};
    if (hipMemsetAsync(c.words, 0, 4 * sizeof(unsigned long long), caller) != hipSuccess || hipEventRecord(n.fork, caller) != hipSuccess ||
        hipStreamWaitEvent(n.stream, n.fork, 0) != hipSuccess) {
      (void)hipGetLastError();
      return -1.f;
    }
    hipLaunchKernelGGL(pipe_probe_hog_kernel, dim3(6144), dim3(256), 0, caller, c.words, 500);
    hipLaunchKernelGGL(pipe_probe_stamp_kernel, dim3(1), dim3(64), 0, n.stream, c.words);
    if (hipEventRecord(n.join, n.stream) != hipSuccess || hipStreamWaitEvent(caller, n.join, 0) != hipSuccess) (void)hipStreamSynchronize(n.stream);
    if (hipStreamSynchronize(caller) != hipSuccess || hipMemcpy(h, c.words, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess || h[0] == 0 || h[1] == 0) {
      (void)hipGetLastError();
      return -1.f;
    }
    return h[1] >= h[0] ? (float)(h[1] - h[0]) / 100.f : 0.f;  // 100 MHz
  }
  static int get(hipStream_t caller, SideStreamHandles* out, const PerDevice::Choice** report = nullptr) {
    PerDevice* c = device_state();
    if (!c) return fail(GP_ERROR_HIP, "SideStream: no current device");
    if (!c->created) create(*c);
    if (c->num == 0) return fail(GP_ERROR_HIP, "SideStream: cannot create the side stream");
    if (c->probed) {
      *out = c->cand[c->chosen.index];
      if (report) *report = &c->chosen;
      return GP_OK;
    }
    PerDevice::Choice pick{caller, 0, {-1.f, -1.f, -1.f, -1.f}};
    c->probed = true;  // (once per thread and device, whatever comes of it)
    if (c->words) {
      for (int i = 0; i < c->num; i++) {
        // (two probes, the smaller delay: a first launch on a new queue pays for the queue)
        const float a = probe(*c, caller, c->cand[i]), b = probe(*c, caller, c->cand[i]);
        pick.delay_us[i] = a < 0.f ? b : b < 0.f ? a : std::min(a, b);
        if (pick.delay_us[i] >= 0.f && (pick.delay_us[pick.index] < 0.f || pick.delay_us[i] < pick.delay_us[pick.index] - 2.f)) pick.index = i;  // (ties within 2 us: the earlier one)
      }
    }
    c->chosen = pick;
    if (report) *report = &c->chosen;
    *out = c->cand[pick.index];
    return GP_OK;
  }
};
void release_side_streams() { SideStream::release(); }  // (gp_trim_device_cache, gp_runtime.hip; declared in gp_host.hpp)
int side_stream_for(hipStream_t caller, SideStreamHandles* out) { return SideStream::get(caller, out); }  // (gp_covariance.hip; declared in gp_host.hpp)
}  // namespace gp

extern "C" {

// measurement / tests: the side stream gp_estimate_covariances uses beside `caller` on the current device -- the delays (us) the pipe probe measured for the (up to four)
// candidate streams (< 0: not probed) and the index of the one in use
int gp_debug_side_stream_probe(gp_stream_t caller, float delays_us[4], int* chosen) {
  gp::SideStreamHandles side;
  const gp::SideStream::PerDevice::Choice* report = nullptr;
  GP_TRY(gp::SideStream::get((hipStream_t)caller, &side, &report));
  for (int i = 0; i < 4; i++)
    if (delays_us) delays_us[i] = report ? report->delay_us[i] : -1.f;
  if (chosen) *chosen = report ? report->index : 0;
  return GP_OK;
}

}  // extern "C"
