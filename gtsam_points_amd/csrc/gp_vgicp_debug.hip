// gp_vgicp_debug.hip -- the check hooks (gp_debug_*) and the measurement entry points of the VGICP path: what a batch measured about itself, the timed kernels of a
// linearise, the trace buffer.  The product's entry points are gp_vgicp_batch.hip; tables and pose staging gp_vgicp_table.hip; the units share gp_vgicp_batch.hpp.
#include "gp_host.hpp"
#include "gp_vgicp_batch.hpp"

// the tiles of a planned launch into the hooks' arrays
static void write_plan_tiles(const gp::StreamPlan& plan, int* begin, int* count) {
  gp::for_each_plan_tile(plan, [&](int t, int b, int c) { begin[t] = b, count[t] = c; });
}

extern "C" {

// timeline hook (measurement): the traced build of the tile kernel of THIS batch's single-factor linearise stores 8 s_memtime stamps + HW_ID /
// XCC_ID + two s_memrealtime stamps per workgroup into dev_buffer ([2048][16] uint64, row = tile index); row 2047 receives the stamps of the
// finalize kernel of synchronous calls.  NULL disables.
int gp_vgicp_batch_set_trace_buffer(gp_vgicp_batch_t* b, void* dev_buffer) {
  if (!b) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_set_trace_buffer: null batch");
  b->trace = static_cast<unsigned long long*>(dev_buffer);
  return GP_OK;
}

// measurement: the by-part fused linearise steps as the device's own 100 MHz clock saw them (batch_linearize_sync reads the stamps), mean per step since the last reset
int gp_vgicp_batch_device_times(gp_vgicp_batch_t* batch, int reset, double* steps, double* stream_us_mean, double* kernel_us_mean) {
  if (!batch) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_device_times: null batch");
  gp_vgicp_measurement& m = batch->measurement;
  if (steps) *steps = m.dev_steps;
  if (stream_us_mean) *stream_us_mean = m.dev_steps > 0 ? m.dev_stream_ticks / m.dev_steps / 100.0 : 0.0;
  if (kernel_us_mean) *kernel_us_mean = m.dev_steps > 0 ? m.dev_kernel_ticks / m.dev_steps / 100.0 : 0.0;
  if (reset) m.dev_steps = m.dev_stream_ticks = m.dev_kernel_ticks = 0.0;
  return GP_OK;
}

// measurement: durations of the tile kernel and the finalize kernel of the last synchronous linearise (GP_TUNE_TIMING = 1), HIP events on the batch's stream
int gp_vgicp_batch_last_kernel_ms(const gp_vgicp_batch_t* batch, float* tile_ms, float* finalize_ms) {
  if (!batch) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_last_kernel_ms: null batch");
  if (tile_ms) *tile_ms = batch->measurement.last_tile_ms;
  if (finalize_ms) *finalize_ms = batch->measurement.last_finalize_ms;
  return GP_OK;
}

int gp_debug_drop_error_words(gp_vgicp_batch_t* b, int count) {
  if (!b || count < 0) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_debug_drop_error_words: a batch and count >= 0");
  b->arrival.drop_error_words = count;
  return GP_OK;
}

// host-side check hook (no device needed): the tiles a planned single-factor launch of n points deals to its workgroups, in tile-list order
// (XCD-major).  begin / count: arrays of `capacity` ints; *num_tiles = workgroups of the launch (<= 1024).
int gp_debug_stream_plan(int n, int skew_permille, const int* xcd_weights_permille, int capacity, int* begin, int* count, int* num_tiles) {
  if (n < 0 || skew_permille < -1 || !num_tiles) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_debug_stream_plan: bad arguments");
  gp::StreamPlan plan;
  const int G = gp::make_stream_plan(n, skew_permille, xcd_weights_permille, &plan);
  *num_tiles = G;
  if (begin && count) {
    if (capacity < G) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_debug_stream_plan: capacity too small");
    write_plan_tiles(plan, begin, count);
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
  const int G = tile_points ? gp::fixed_tile_count(n, tile_points) : gp::make_stream_plan(n, skew_permille, xcd_weights_permille, &plan, max_workgroups);
  *num_tiles = G;
  if (!begin || !count) return GP_OK;
  if (capacity < G) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_debug_stream_plan_ex: capacity too small");
  if (tile_points) {
    for (int t = 0; t < G; t++) gp::fixed_tile(t, n, tile_points, &begin[t], &count[t]);
  } else {
    write_plan_tiles(plan, begin, count);
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
  gp::expand_rigid_host(sums, pose, reinterpret_cast<double*>(out));
  return GP_OK;
}

int gp_vgicp_batch_time_linearize(gp_vgicp_batch_t* b, const double* poses_host, int iters, float* ms_total, float* ms_main_kernel, float* ms_finalize_kernel) {
  if (!b || !poses_host || iters <= 0) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_time_linearize: bad arguments");
  GP_TRY(gp::ensure_table(b));
  const size_t F = b->factors.size();
  if (F == 0) return GP_OK;
  // the device work of the SYNCHRONOUS call (gp_vgicp_batch_linearize), incl. its split finalize for a single large factor
  const bool rigid = gp::takes_rigid_path(b, poses_host);
  const int parts = gp::linearize_parts(b, rigid);
  gp::DeviceArray d_out;
  GP_TRY(d_out.alloc(sizeof(gp_linearized6) * F * (size_t)parts));
  gp::PoseSource ps;
  GP_TRY(gp::stage_poses(b, poses_host, nullptr, &ps));
  double* partials = nullptr;
  GP_TRY(gp::partials_ptr(b, &partials));
  hipEvent_t e0, e1, e2;
  GP_HIP(hipEventCreate(&e0));
  GP_HIP(hipEventCreate(&e1));
  GP_HIP(hipEventCreate(&e2));
  GP_TRY(gp::launch_linearize(b, ps, d_out.as<gp_linearized6>(), rigid, {}, parts));  // warm-up
  GP_HIP(hipStreamSynchronize(b->stream));
  // whole pass, back to back
  GP_HIP(hipEventRecord(e0, b->stream));
  for (int i = 0; i < iters; i++) GP_TRY(gp::launch_linearize(b, ps, d_out.as<gp_linearized6>(), rigid, {}, parts));
  GP_HIP(hipEventRecord(e1, b->stream));
  GP_HIP(hipEventSynchronize(e1));
  float t_total = 0.f;
  GP_HIP(hipEventElapsedTime(&t_total, e0, e1));
  // main kernel alone, then finalize alone (same stream the product path launches on)
  GP_HIP(hipEventRecord(e0, b->stream));
  for (int i = 0; i < iters; i++) GP_TRY(rigid ? gp::launch_tiles<gp::MODE_LIN>(b, ps, partials) : gp::launch_tiles<gp::MODE_LIN_GENERAL>(b, ps, partials));
  GP_HIP(hipEventRecord(e1, b->stream));
  for (int i = 0; i < iters; i++)
    GP_TRY(rigid ? gp::launch_finalize<false>(b, ps, partials, d_out.as<gp_linearized6>(), {}, parts) : gp::launch_finalize<true>(b, ps, partials, d_out.as<gp_linearized6>()));
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
