// gp_vgicp_plan.hpp -- the host arithmetic of the VGICP batch that touches no device: how a planned single-factor launch of the stream kernel deals its chunks
// (make_stream_plan; gp_debug_stream_plan shows the result) and the 6x6 expansion of the rigid finalize's 32 sums (expand_rigid_host; gp_debug_expand_rigid).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "gp_vgicp_shared.hpp"

namespace gp {

constexpr int kResidentWorkgroups = 1024;  // 256 compute units x 4 workgroups of the tile kernels (34-40 KB of LDS, <= 128 VGPRs)
constexpr int kDefaultSkewPermille = -1;  // automatic: by the mean share (make_stream_plan)

// Stream kernel, ONE large factor of n points: the launch geometry (number of workgroups, a multiple of 8) and how the chunks are dealt
// (StreamPlan, gp_vgicp_shared.hpp).  At most one resident round of workgroups whatever n is.
//   skew_permille   how much more a dispatch round takes than the next one, in 1/1000 of the mean share (0 = flat split)
//   xcd_weights     per-XCD share in 1/1000 of the mean share (1000 = equal), or null = kXcdWeightPermille
// Measured on MI355X (round 4, scripts/r04_instep_xcd.py: per-workgroup start / end stamps of the 1 M-point headline INSIDE synchronous steps, i.e. behind
// an idle queue -- the pattern every synchronous call runs in): the command processor hands the dispatch to the XCDs one after the other, in the order
// 0, 1, 2, 3, 7, 6, 5, 4: XCD 1 starts 0.17 us behind XCD 0, XCD 3 0.5 us, XCD 7 0.6-0.9, XCD 4 1.1-1.5 us (two boxes) -- and with equal shares they END
// as much later: XCDs 0-3 at 10.4-11.3 us, XCD 4 at 12.8.  (Back to back the offsets are 0.3-0.7 us, which is why round 3's weights, measured back
// to back, moved nothing.)  A workgroup's life is ~3.7 us of fill and drain + ~6 us that scale with its share, so the shares that equalise the ends are
// 1 + (mean offset - offset) / 6 us: the table below (mean of the two boxes' offsets).  Last end 12.8 -> 11.8-11.9 us in the traced build.
// GP_TUNE_XCD_WEIGHT_0 + x overrides.
constexpr int kXcdWeightPermille[gp::kNumXCD] = {1090, 1070, 1045, 1025, 905, 935, 950, 980};
// waves = waves per workgroup: 4 in the product; the 8- / 16-wave geometries of round 6 (gp_vgicp_stream.hpp, W) were planned through the same function
inline int make_stream_plan(int n, int skew_permille, const int* xcd_weights, gp::StreamPlan* p, int max_wgs = kResidentWorkgroups, int waves = 4) {
  const int C = n / gp::kChunkPoints;
  max_wgs = std::min(max_wgs, kResidentWorkgroups * 4 / waves);  // one resident round: 16 waves per compute unit
  const int G = std::min(std::max(gp::kNumXCD, max_wgs / gp::kNumXCD * gp::kNumXCD), (std::max((C + waves - 1) / waves, 1) + gp::kNumXCD - 1) / gp::kNumXCD * gp::kNumXCD);
  const int gx = G / gp::kNumXCD;
  *p = gp::StreamPlan{};
  p->tail = n % gp::kChunkPoints;
  p->wgs_per_xcd = gx;
  const double mean_chunks = (double)C / G;
  if (skew_permille < 0) {
    // automatic.  Round 3 needed ~250 at 15 chunks per workgroup because the rounds also had to absorb the XCDs' start offsets; with those in the XCD shares
    // (below) the in-step sweeps of round 4 (scripts/r04_sweep.py, 1 M / 3 M / 8 M points) put the best value at 100-150 for every size: 250 costs 0.3-0.5 us at
    // 1 M and 3 us at 8 M, 50 as much
    skew_permille = 150;
  }
  // shares of the XCDs: proportional to their weights, whole chunks, summing to C (largest remainders first; equal weights = cx or cx + 1).
  // The library's table compensates a FIXED delay (the XCD's dispatch offset), measured at the headline's 15.26 chunks per workgroup: its deviations from 1000
  // scale with 15.26 / (chunks per workgroup) -- an 8 M-point source gets an eighth of them (the unscaled table cost it 1.5 us of 60), a 100 k-point one twice.
  int scaled[gp::kNumXCD];
  if (!xcd_weights) {
    const double k = std::min(2.0, 15.26 / std::max(mean_chunks, 1.0));
    for (int x = 0; x < gp::kNumXCD; x++) scaled[x] = 1000 + (int)std::lround((kXcdWeightPermille[x] - 1000) * k);
  }
  const int* w = xcd_weights ? xcd_weights : scaled;
  int share[gp::kNumXCD];
  {
    int64_t wsum = 0;
    for (int x = 0; x < gp::kNumXCD; x++) wsum += std::max(w[x], 1);
    int given = 0;
    int64_t frac[gp::kNumXCD];
    for (int x = 0; x < gp::kNumXCD; x++) {
      const int64_t num = (int64_t)C * std::max(w[x], 1);
      share[x] = (int)(num / wsum);
      frac[x] = num % wsum;
      given += share[x];
    }
    for (int left = C - given; left > 0; left--) {
      int best = 0;
      for (int x = 1; x < gp::kNumXCD; x++)
        if (frac[x] > frac[best]) best = x;
      share[best]++;
      frac[best] = -1;
    }
  }
  for (int x = 0, at = 0; x < gp::kNumXCD; x++) {
    p->xbegin[x] = at;
    at += share[x];
  }
  const int rounds = (gx + gp::kStreamRound - 1) / gp::kStreamRound;  // <= 4
  const int late = gx - gp::kStreamRound * (rounds - 1);
  auto fill = [&](int x, double skew) {  // shares of the rounds of XCD x in front of its last one; returns what the last round's workgroups share
    const double mean = (double)share[x] / gx;
    int used = 0;
    for (int r = 0; r < 3; r++) p->n[x][r] = p->pre[x][r] = 0;
    for (int r = 0; r + 1 < rounds; r++) {
      p->n[x][r] = std::max(0, (int)std::ceil(mean * (1.0 + skew * (0.5 * (rounds - 1) - r)) - 1e-9));  // (rounded up: the last round never ends up above the one before it)
      p->pre[x][r] = used;
      used += gp::kStreamRound * p->n[x][r];
    }
    p->before_last[x] = used;
    return share[x] - used;
  };
  // the last round must get something sensible on every XCD: at least a third of the mean share per workgroup, never a negative rest; else
  // (and for skew 0) ONE flat round per XCD: every workgroup floor(share / gx) chunks, the first share % gx one more
  bool skewed = skew_permille > 0 && rounds > 1;
  for (int x = 0; x < gp::kNumXCD && skewed; x++) {
    const int rem = fill(x, skew_permille / 1000.0);
    if (rem < 0 || (int64_t)rem * 3 * gx < (int64_t)share[x] * late) skewed = false;
  }
  p->last_begin = skewed ? gp::kStreamRound * (rounds - 1) : 0;
  if (!skewed)
    for (int x = 0; x < gp::kNumXCD; x++) {
      for (int r = 0; r < 3; r++) p->n[x][r] = p->pre[x][r] = 0;
      p->before_last[x] = 0;
    }
  const int late_wgs = gx - p->last_begin;
  for (int x = 0; x < gp::kNumXCD; x++) {
    const int left = share[x] - p->before_last[x];
    p->lo[x] = left / late_wgs;
    p->extra[x] = left % late_wgs;
  }
  return G;
}

// the tiles of a planned launch in tile-list order (XCD-major), as plan_tile deals them: fn(t, begin, count).  build_table() stores these,
// gp_debug_stream_plan[_ex] shows them.
template <class Fn>
inline void for_each_plan_tile(const gp::StreamPlan& plan, Fn&& fn) {
  int t = 0;
  for (int x = 0; x < gp::kNumXCD; x++)
    for (int q = 0; q < plan.wgs_per_xcd; q++, t++) {
      int begin = 0, count = 0;
      gp::plan_tile(gp::plan_fields(plan, x, q), x, q, &begin, &count);
      fn(t, begin, count);
    }
}

// Fixed tiles (every batch, and a single factor below the planning threshold): a factor of n points is cut into tiles of tile_points, the last one partial.
// build_table() fills the tile table with these, gp_debug_stream_plan_ex shows them.
inline int fixed_tile_count(int n, int tile_points) { return (n + tile_points - 1) / tile_points; }
inline void fixed_tile(int t, int n, int tile_points, int* begin, int* count) {
  *begin = t * tile_points;
  *count = std::min(tile_points, n - t * tile_points);
}

// the 6x6 expansion of the rigid finalize kernel on the host (same formulas: H_t from the 29 sums, Ad(delta), H_ts = -H_t Ad, H_s = Ad^T H_t Ad,
// b_s = -Ad^T b_t): used by the synchronous single-factor call, whose finalize parts then deliver only their sums
inline void expand_rigid_host(const double* sum, const double* pose /*col-major 4x4*/, double* dst /*[122]*/) {
  constexpr int OFF_HT = 2, OFF_HS = 38, OFF_HTS = 74, OFF_BT = 110, OFF_BS = 116;
  const double Rl[9] = {pose[0], pose[4], pose[8], pose[1], pose[5], pose[9], pose[2], pose[6], pose[10]};  // row-major R
  const double tx = pose[12], ty = pose[13], tz = pose[14];
  const double Xl[9] = {0.0, -tz, ty, tz, 0.0, -tx, -ty, tx, 0.0};  // [t]x, row-major
  auto sym3 = [](int a, int b) {
    const int i = a < b ? a : b, j = a < b ? b : a;
    return (i * (5 - i)) / 2 + j;
  };
  double Ht[6][6], Ad[6][6], HtA[6][6], bt[6];
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) {
      double h;
      if (r < 3 && c < 3) h = sum[gp::ACC_TL + sym3(r, c)];
      else if (r >= 3 && c < 3) h = -sum[gp::ACC_K + (r - 3) * 3 + c];
      else if (r < 3) h = -sum[gp::ACC_K + (c - 3) * 3 + r];
      else h = sum[gp::ACC_M + sym3(r - 3, c - 3)];
      Ht[r][c] = h;
      dst[OFF_HT + c * 6 + r] = h;
      double a;
      if (r < 3 && c < 3) a = Rl[r * 3 + c];
      else if (r < 3) a = 0.0;
      else if (c >= 3) a = Rl[(r - 3) * 3 + (c - 3)];
      else a = Xl[(r - 3) * 3] * Rl[c] + Xl[(r - 3) * 3 + 1] * Rl[3 + c] + Xl[(r - 3) * 3 + 2] * Rl[6 + c];
      Ad[r][c] = a;
    }
  for (int k = 0; k < 6; k++) {
    bt[k] = k < 3 ? sum[gp::ACC_QXMR + k] : sum[gp::ACC_MR + k - 3];
    dst[OFF_BT + k] = bt[k];
  }
  dst[0] = sum[gp::ACC_COUNT];
  dst[1] = sum[gp::ACC_ERR];
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) {
      double a = 0.0;
      for (int k = 0; k < 6; k++) a += Ht[r][k] * Ad[k][c];
      HtA[r][c] = a;
      dst[OFF_HTS + c * 6 + r] = -a;
    }
  for (int k6 = 0; k6 < 6; k6++) {
    double a = 0.0;
    for (int k = 0; k < 6; k++) a += Ad[k][k6] * bt[k];
    dst[OFF_BS + k6] = -a;
  }
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) {
      double a = 0.0;
      for (int k = 0; k < 6; k++) a += Ad[k][r] * HtA[k][c];
      dst[OFF_HS + c * 6 + r] = a;
    }
}

}  // namespace gp
