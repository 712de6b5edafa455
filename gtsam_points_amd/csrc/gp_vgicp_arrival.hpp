// gp_vgicp_arrival.hpp -- the arrival protocol of the fused finalize, host side (the device side is gp_vgicp_stream.hpp).  A fused call is ONE launch: the tile
// workgroups count themselves in at arrival counters, and the one that completes a count -- of a PART of a large factor's tile list, or of a FACTOR -- sums the rows
// and hands result and completion word to the host.  A call has two halves:
//   launch_fused_parts / launch_fused_factors   arm the counters, launch the tiles, commit what the counters will read (or write the empty factors' slots);
//   finish_fused                                wait for the words; if they are missing, start the counters of that form over, run the call's sums again through
//                                               the caller's two-kernel fallback and wait for its words.
// Included by the unit that holds the synchronous entry points (gp_vgicp_batch.hip).
#pragma once

#include <algorithm>
#include <cstring>

#include "gp_vgicp_batch.hpp"

namespace gp {
#pragma GCC visibility push(hidden)

// how long a synchronous call polls its completion words before it hands over to hipStreamSynchronize: 100 us + 50 ps per source point
// (4x what the tile kernel takes), so that a healthy pass never gets there
inline long spin_budget_us(const gp_vgicp_batch* b) { return 100 + (long)(b->total_points / 20000); }

// every synchronous call ends here: poll `count` completion words for `seq` (gp::wait_done), within the call's spin budget
inline int wait_words(gp_vgicp_batch* b, size_t count, unsigned long long seq, long extra_spin_us = 0) {
  return wait_done(static_cast<const unsigned long long*>(b->arrival.h_done.ptr), count, seq, b->stream, spin_budget_us(b) + extra_spin_us);
}

// the completion words of the batch's next call
inline DoneFlags next_done(gp_vgicp_batch* b, unsigned long long* trace = nullptr) {
  return DoneFlags{static_cast<unsigned long long*>(b->arrival.h_done_dev), ++b->arrival.seq, trace};
}

// gp_debug_drop_error_words: this fused error evaluation is to read as if its completion words had not arrived (host side only: the kernels run as always)
inline bool take_dropped_error_words(gp_vgicp_batch* b) {
  if (b->arrival.drop_error_words <= 0) return false;
  b->arrival.drop_error_words--;
  return true;
}

// did every part's completion word arrive?  (after wait_done, which hands over to hipStreamSynchronize when its spin budget is used up: in the two-kernel
// form a finished stream means finished records, in the fused form the records exist only if the parts' last workgroups saw their counters complete)
inline bool words_arrived(const gp_vgicp_batch* b, size_t count, unsigned long long seq) {
  const volatile unsigned long long* fl = static_cast<const volatile unsigned long long*>(b->arrival.h_done.ptr);
  for (size_t g = 0; g < count; g++)
    if (fl[g] != seq) return false;
  return true;
}

inline int rows_per_part(const gp_vgicp_batch* b, int parts) { return (b->num_tiles + parts - 1) / parts; }

// where the last workgroups deliver, common to both forms
inline void arm_delivery(gp_vgicp_batch* b, PoseSource* ps, unsigned long long* counters, int rows_per_part, int fin_stride, const DoneFlags& done) {
  ps->inl.arrive = counters;
  ps->inl.rows_per_part = rows_per_part;
  ps->inl.num_rows = b->num_tiles;
  ps->inl.fin_out = static_cast<double*>(b->h_out_dev);
  ps->inl.fin_stride = fin_stride;
  ps->inl.fin_flags = done.flags;
  ps->inl.fin_seq = done.seq;
}

// fused finalize by PART: ONE launch, the last workgroup of each part of the tile list finalizes the part (gp_vgicp_stream.hpp: finalize_part_rows) into slot g of
// h_out (a record apart) and completion word g.  Arrival counters: monotonic, one per part, kArriveStride words apart; the host's count of them is committed once
// the launch has gone out.  *partials = the launch's rows.
template <int MODE>
int launch_fused_parts(gp_vgicp_batch* b, PoseSource* ps, int parts, const DoneFlags& done, double** partials) {
  gp_vgicp_arrival& a = b->arrival;
  GP_TRY(partials_ptr(b, partials));
  if (!a.d_arrive.ptr) {
    GP_TRY(a.d_arrive.alloc(sizeof(unsigned long long) * 16 * kArriveStride));
    GP_HIP(hipMemset(a.d_arrive.ptr, 0, sizeof(unsigned long long) * 16 * kArriveStride));
    memset(a.arrived, 0, sizeof(a.arrived));
  }
  const int per = rows_per_part(b, parts);
  arm_delivery(b, ps, a.d_arrive.as<unsigned long long>(), per, (int)(sizeof(gp_linearized6) / sizeof(double)), done);
  for (int g = 0; g < parts; g++) ps->inl.arrive_target[g] = a.arrived[g] + (unsigned long long)std::max(0, std::min(per, b->num_tiles - g * per));
  GP_TRY(launch_tiles<MODE>(b, *ps, *partials));
  for (int g = 0; g < parts; g++) a.arrived[g] = ps->inl.arrive_target[g];
  return GP_OK;
}

// fused finalize by FACTOR: ONE launch, the workgroup that stores a factor's last row finalizes the factor (gp_vgicp_stream.hpp) and hands slot i of fin_out (fin_stride
// doubles apart: a record, or one double of an error evaluation) and completion word i to the host.  One zero-reset counter per factor (the last arriver of a factor
// stores 0): a launch that went out and was never seen to complete (an error return between launch and the last completion word, a torn-down kernel) may have left
// small positive values behind, which would let the NEXT launch's factors finalize early on stale rows without anybody noticing.  Such a batch cleans its
// counters, behind the stream, before it counts again: factor_arrive_dirty stays set until finish_fused has seen every completion word of THIS launch.
// A factor without points has no workgroup to finalize it: its slot and its completion word are written here.  poses_host: the linearise's poses (the empty record is
// the expansion of zero sums at the factor's pose); null: an error evaluation (the empty sum).
template <int MODE>
int launch_fused_factors(gp_vgicp_batch* b, PoseSource* ps, const double* poses_host, const DoneFlags& done, double** partials) {
  gp_vgicp_arrival& a = b->arrival;
  const size_t F = b->factors.size();
  if (a.factor_arrive_count < F) {
    const size_t bytes = sizeof(unsigned long long) * kFactorArriveStride * F;
    GP_TRY(a.d_factor_arrive.alloc(bytes));
    GP_HIP(hipMemset(a.d_factor_arrive.ptr, 0, bytes));
    a.factor_arrive_count = F;
  }
  GP_TRY(partials_ptr(b, partials));
  if (a.factor_arrive_dirty) {
    GP_HIP(hipStreamSynchronize(b->stream));
    GP_HIP(hipMemset(a.d_factor_arrive.ptr, 0, sizeof(unsigned long long) * kFactorArriveStride * a.factor_arrive_count));
    a.factor_arrive_dirty = false;
  }
  arm_delivery(b, ps, a.d_factor_arrive.as<unsigned long long>(), 0, MODE == MODE_ERR ? 1 : (int)(sizeof(gp_linearized6) / sizeof(double)), done);
  a.factor_arrive_dirty = true;
  GP_TRY(launch_tiles<MODE>(b, *ps, *partials));
  for (size_t i = 0; i < F; i++)
    if (b->h_descs[i].tile_count == 0) {
      if (poses_host) {
        const double zeros[32] = {0.0};
        expand_rigid_host(zeros, poses_host + 16 * i, reinterpret_cast<double*>(static_cast<gp_linearized6*>(b->h_out.ptr) + i));
      } else {
        static_cast<volatile double*>(b->h_out.ptr)[i] = 0.0;
      }
      static_cast<volatile unsigned long long*>(a.h_done.ptr)[i] = done.seq;
    }
  return GP_OK;
}

enum class Arrival { by_part, by_factor };

// The second half of a fused call: wait for its `words` completion words.  When the stream is idle and words are missing, the device's counters and the host's idea of
// them have come apart (a launch that failed half way, a kernel that was torn down, a counter left dirty).  The rows are complete, so the counters of that form start
// over from zero and fallback(again) does the call's sums again in the two-kernel form, which announces itself with the words `again`.
//   error_eval     a fused error evaluation consults the drop hook (gp_debug_drop_error_words), once, between the wait and the look at the words
//   queued_behind  the caller returned between launch and wait (_begin / _end) and more work may stand on the stream: 400 us more spin (the damped step queued in
//                  front of it), and the stream is drained before the counters are touched
//   recovered      if given: did the fallback run?
// An error return leaves factor_arrive_dirty set.
template <class Fallback>
int finish_fused(gp_vgicp_batch* b, Arrival form, size_t words, unsigned long long seq, bool error_eval, Fallback&& fallback, bool* recovered = nullptr,
                 bool queued_behind = false) {
  gp_vgicp_arrival& a = b->arrival;
  GP_TRY(wait_words(b, words, seq, queued_behind ? 400 : 0));
  const bool dropped = error_eval && take_dropped_error_words(b);
  const bool missing = dropped || !words_arrived(b, words, seq);
  if (missing) {
    if (queued_behind) GP_HIP(hipStreamSynchronize(b->stream));
    if (form == Arrival::by_factor) {
      GP_HIP(hipMemset(a.d_factor_arrive.ptr, 0, sizeof(unsigned long long) * kFactorArriveStride * b->factors.size()));
    } else {
      GP_HIP(hipStreamSynchronize(b->stream));
      if (a.d_arrive.ptr) GP_HIP(hipMemset(a.d_arrive.ptr, 0, sizeof(unsigned long long) * 16 * kArriveStride));
      memset(a.arrived, 0, sizeof(a.arrived));
    }
    const DoneFlags again = next_done(b);
    GP_TRY(fallback(again));
    GP_TRY(wait_words(b, words, again.seq));
  }
  if (form == Arrival::by_factor) a.factor_arrive_dirty = false;  // every factor's last arriver reset its counter (or the recovery cleaned them)
  if (recovered) *recovered = missing;
  return GP_OK;
}

#pragma GCC visibility pop
}  // namespace gp
