// gp_vgicp.hip -- fused VGICP linearisation / error evaluation for gfx950, single-factor and batched.
//
// Replaces (reference):
//   include/gtsam_points/cuda/kernels/{lookup_voxels,vgicp_derivatives,linearized_system}.cuh  (device functors)
//   src/gtsam_points/factors/integrated_vgicp_derivatives{,_linearize,_compute,_inliers}.cu       (CUB reduce / select)
//   the per-factor launch loop of src/gtsam_points/cuda/nonlinear_factor_set_gpu.cpp:64-218
//
// Shape of the computation:
//   main kernel    : one 256-thread workgroup per TILE of kTilePoints consecutive source points of one factor.
//                    per point: q = R p + t (f64) -> floor -> hash probe (16-B bucket) -> 64-B voxel record ->
//                    M = (C_B + R C_A R^T)^-1 -> 29 target-side sums; 64-lane shuffle reduce, LDS cross-wave
//                    reduce, ONE 32-double partial per tile.  No atomics, no inlier list, no CUB temp storage.
//   finalize kernel: one workgroup per factor sums its tiles' partials in a fixed order (deterministic) and
//                    expands them to the LinearizedSystem6 blocks through the adjoint identity
//                    J_s = -J_t Ad(delta):  H_s = Ad^T H_t Ad, H_ts = -H_t Ad, b_s = -Ad^T b_t.
// This unit defines and launches the kernels; the batch, its tables, the arrival protocol of the fused finalize and the C entry points are gp_vgicp_batch.hip.
//   The workgroup -> tile map is XCD-aware: workgroup b runs on XCD b % 8, so XCD x is handed the x-th contiguous
//   eighth of the tile list and the voxel tables of "its" factors stay in that XCD's 4 MiB L2.
#include <atomic>
#include <chrono>
#include <cstring>

#include "gp_host.hpp"
#include "gp_vgicp_batch.hpp"
#include "gp_vgicp_tile.hpp"
#include "gp_vgicp_tile2.hpp"
#include "gp_vgicp_finalize.hpp"
#include "gp_vgicp_stream.hpp"

namespace gp {

template <int MODE>
struct ModeTraits {
  static constexpr int kAcc = MODE == MODE_ERR ? 2 : (MODE == MODE_LIN ? ACC_SIZE : ACCG_SIZE);
  static constexpr int kStride = MODE == MODE_LIN_GENERAL ? ACCG_STRIDE : ACC_STRIDE;
};

template <int MODE>
__device__ __forceinline__ void accumulate_point(const FactorDesc& f, const Pose& Tl, const Pose& Te, int i, double* acc) {
  const float* __restrict__ pp = f.points + 3 * (size_t)i;
  const double px = (double)pp[0], py = (double)pp[1], pz = (double)pp[2];
  if (!finite3(px, py, pz)) return;  // a NaN / inf return has no voxel
  // correspondence at the LINEARISATION pose (lookup kernel is built with d_xl, integrated_vgicp_derivatives_compute.cu:25)
  const double lx = Tl.r00 * px + Tl.r01 * py + Tl.r02 * pz + Tl.tx;
  const double ly = Tl.r10 * px + Tl.r11 * py + Tl.r12 * pz + Tl.ty;
  const double lz = Tl.r20 * px + Tl.r21 * py + Tl.r22 * pz + Tl.tz;
  if (f.surface_validation && surface_rejected(Tl, lx, ly, lz, f.normals + 3 * (size_t)i)) return;
  const int cx = fast_floor(lx * f.map.inv_leaf), cy = fast_floor(ly * f.map.inv_leaf), cz = fast_floor(lz * f.map.inv_leaf);
  const int v = lookup_voxel(f.map, cx, cy, cz);
  if (v < 0) return;

  // one 64-B gather: {mean_local f32x3, n, cov f64x6}
  const VoxelRecord* __restrict__ rec = f.map.records + v;
  const float4 head = *reinterpret_cast<const float4*>(rec);
  const double2 c01 = *reinterpret_cast<const double2*>(rec->cov);
  const double2 c23 = *reinterpret_cast<const double2*>(rec->cov + 2);
  const double2 c45 = *reinterpret_cast<const double2*>(rec->cov + 4);
  const double cb[6] = {c01.x, c01.y, c23.x, c23.y, c45.x, c45.y};

  const float* __restrict__ cp = f.covs + 9 * (size_t)i;
  // symmetric part of the column-major 3x3 (exactly the input when it is symmetric)
  const double ca[6] = {(double)cp[0], 0.5 * ((double)cp[3] + (double)cp[1]), 0.5 * ((double)cp[6] + (double)cp[2]),
                        (double)cp[4], 0.5 * ((double)cp[7] + (double)cp[5]), (double)cp[8]};

  double m[6];
  fused_mahalanobis(Tl, ca, cb, m);

  double ox, oy, oz;
  voxel_center(f.map, cx, cy, cz, ox, oy, oz);
  double qx, qy, qz;
  if constexpr (MODE == MODE_ERR) {
    qx = Te.r00 * px + Te.r01 * py + Te.r02 * pz + Te.tx;
    qy = Te.r10 * px + Te.r11 * py + Te.r12 * pz + Te.ty;
    qz = Te.r20 * px + Te.r21 * py + Te.r22 * pz + Te.tz;
  } else {
    qx = lx;
    qy = ly;
    qz = lz;
  }
  // r = mu_B - q, with mu_B = centre + mean_local
  const double rx = (ox - qx) + (double)head.x;
  const double ry = (oy - qy) + (double)head.y;
  const double rz = (oz - qz) + (double)head.z;
  accumulate_sums<MODE>(Tl, m, px, py, pz, qx, qy, qz, rx, ry, rz, acc);
}

// main kernel: one workgroup per tile; writes partials[tile][kStride]
template <int MODE>
__global__ void __launch_bounds__(kBlockThreads) vgicp_tile_kernel(const FactorDesc* __restrict__ factors, const TileDesc* __restrict__ tiles, int num_tiles,
                                                                   const double* __restrict__ poses_lin, const double* __restrict__ poses_eval,
                                                                   const InlinePoses inl, double* __restrict__ partials) {
  constexpr int NACC = ModeTraits<MODE>::kAcc;
  constexpr int STRIDE = ModeTraits<MODE>::kStride;
  const int tile_idx = xcd_swizzle(blockIdx.x, num_tiles);
  if (tile_idx >= num_tiles) return;
  TileDesc tile;
  if (inl.use) {
    tile.factor = 0;
    if (inl.tile_points > 0) {
      tile.begin = tile_idx * inl.tile_points;
      tile.count = min(inl.tile_points, inl.factor.n - tile.begin);
    } else {  // the table of a single-factor stream batch is its plan (gp_vgicp_stream.hpp): tiles of different sizes, XCD-major
      const int px = tile_idx / inl.plan.wgs_per_xcd, pq = tile_idx % inl.plan.wgs_per_xcd;
      plan_tile(plan_fields(inl.plan, px, pq), px, pq, &tile.begin, &tile.count);
    }
    tile.row = tile_idx;
  } else {
    tile = tiles[tile_idx];
  }
  const FactorDesc f = inl.use ? inl.factor : factors[tile.factor];
  const Pose Tl = inl.use ? load_pose(inl.lin) : load_pose(poses_lin + 16 * (size_t)tile.factor);
  const Pose Te = MODE == MODE_ERR ? (inl.use ? load_pose(inl.eval) : load_pose(poses_eval + 16 * (size_t)tile.factor)) : Tl;

  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; k++) acc[k] = 0.0;

  for (int local = threadIdx.x; local < tile.count; local += kBlockThreads) accumulate_point<MODE>(f, Tl, Te, tile.begin + local, acc);

  // 64-lane wavefront reduction
#pragma unroll
  for (int k = 0; k < NACC; k++) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    acc[k] = v;
  }
  __shared__ double lds[kBlockThreads / 64][STRIDE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NACC; k++) lds[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < STRIDE) {
    double s = 0.0;
    if (threadIdx.x < NACC) {
#pragma unroll
      for (int w = 0; w < kBlockThreads / 64; w++) s += lds[w][threadIdx.x];
    }
    partials[(size_t)tile.row * STRIDE + threadIdx.x] = s;
  }
}

// finalize: one workgroup per factor; deterministic ordered sum of the factor's tile partials, then expansion to the
// LinearizedSystem6 blocks.  The 92 explicit sums (ACCG layout): the source-side blocks are read directly, no adjoint identity.
constexpr int kFinalizeThreads = 1024;

__global__ void __launch_bounds__(kFinalizeThreads) vgicp_finalize_general_kernel(const FactorDesc* __restrict__ factors, const InlinePoses inl,
                                                                                  const double* __restrict__ partials, gp_linearized6* __restrict__ out,
                                                                                  const DoneFlags done) {
  constexpr int STRIDE = ACCG_STRIDE;
  constexpr int kSlices = kFinalizeThreads / STRIDE;  // 1024 threads = 10 slices x 96 sums (+ idle)
  const int fi = blockIdx.x;
  const int tile_begin = inl.use ? inl.factor.tile_begin : factors[fi].tile_begin;
  const int tile_count = inl.use ? inl.factor.tile_count : factors[fi].tile_count;
  __shared__ double lds[kSlices][STRIDE];
  __shared__ double sum[STRIDE];
  GP_FIN_TRACE(0);
  if (done.trace && threadIdx.x == 0 && blockIdx.x == 0) done.trace[9] = __builtin_amdgcn_s_getreg(GP_GETREG_XCC_ID);
  const int comp = threadIdx.x % STRIDE, slice = threadIdx.x / STRIDE;
  if (slice < kSlices) {
    // fixed summation order (deterministic).  All of a lane's rows are requested in ONE batch of up to 32 independent loads
    // (the rows were written by workgroups on other XCDs, so every load is an L2 miss: round trips, not bytes, set the time)
    const double* base = partials + (size_t)tile_begin * STRIDE + comp;
    double total = 0.0;
    for (int t0 = slice; t0 < tile_count; t0 += 32 * kSlices) {
      double v[32];
#pragma unroll
      for (int k = 0; k < 32; k++) {
        const int t = t0 + k * kSlices;
        v[k] = t < tile_count ? base[(size_t)t * STRIDE] : 0.0;
      }
#pragma unroll
      for (int w = 16; w > 0; w >>= 1) {
#pragma unroll
        for (int k = 0; k < w; k++) v[k] += v[k + w];
      }
      total += v[0];
    }
    lds[slice][comp] = total;
  }
  GP_FIN_TRACE(1);
  __syncthreads();
  if (threadIdx.x < STRIDE) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < kSlices; k++) a += lds[k][threadIdx.x];
    sum[threadIdx.x] = a;
  }
  __syncthreads();
  GP_FIN_TRACE(2);
  const int t = threadIdx.x;
  const int r = t / 6, c = t % 6;  // t < 36: one 6x6 entry per lane
  // the record is assembled in LDS and leaves in one coalesced sweep of 8-byte stores at the end: when `out` is host-mapped
  // memory, ~130 scattered stores would each be their own PCIe write
  __shared__ double dst[122];
  double* out_rec = reinterpret_cast<double*>(out + fi);  // may be only 8-byte aligned (integrated_vgicp_factor_gpu.cpp:219-220)
  constexpr int OFF_HT = 2, OFF_HS = 38, OFF_HTS = 74, OFF_BT = 110, OFF_BS = 116;
  if (t < 36) {
    // H_t = [[TL, -K^T], [-K, M]]
    const int sym3[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    double h;
    if (r < 3 && c < 3) {
      h = sum[ACC_TL + sym3[r][c]];
    } else if (r >= 3 && c < 3) {
      h = -sum[ACC_K + (r - 3) * 3 + c];
    } else if (r < 3) {
      h = -sum[ACC_K + (c - 3) * 3 + r];
    } else {
      h = sum[ACC_M + sym3[r - 3][c - 3]];
    }
    dst[OFF_HT + c * 6 + r] = h;
  }
  if (t < 6) {
    const double b = t < 3 ? sum[ACC_QXMR + t] : sum[ACC_MR + t - 3];
    dst[OFF_BT + t] = b;
  }
  if (t == 0) {
    dst[0] = sum[ACC_COUNT];
    dst[1] = sum[ACC_ERR];
  }
  __syncthreads();
  if (t < 36) {
    const int sym3[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    double h;
    if (r < 3 && c < 3) {
      h = sum[ACCG_HS_TL + sym3[r][c]];
    } else if (r >= 3 && c < 3) {
      h = sum[ACCG_HS_BL + (r - 3) * 3 + c];
    } else if (r < 3) {
      h = sum[ACCG_HS_BL + (c - 3) * 3 + r];
    } else {
      h = sum[ACCG_HS_BR + sym3[r - 3][c - 3]];
    }
    dst[OFF_HS + c * 6 + r] = h;
    dst[OFF_HTS + c * 6 + r] = sum[ACCG_HTS + r * 6 + c];
  }
  if (t < 6) dst[OFF_BS + t] = sum[ACCG_BS + t];
  __syncthreads();
  GP_FIN_TRACE(3);
  if (t < 122) out_rec[t] = dst[t];
  signal_done(done, fi, t < 122);
}

// finalize of the 29-sum (rigid pose) pass, round 2.  The timeline of the generic kernel above (scripts/trace_finalize.py) showed
// 2.7 us for the partials (250 KB through ONE compute unit's L1: bandwidth, not latency), and then 2.1 + 2.4 us for what should be
// nothing: sixteen waves meeting at four barriers, 6x6 tables indexed at run time (= scratch memory round trips) and a pose fetched
// when it was needed.  Here all sixteen waves load and tree-add their rows, the two slices of a wave meet through one cross-lane
// add, ONE barrier, and wave 0 alone does the rest out of LDS with wave-level synchronisation; the pose is requested first of all.
// THREADS: 1024 (one workgroup sums all the tiles of a factor) or 256 (the split form: an eighth of a large factor's tiles per workgroup --
// four waves meet at the barrier instead of sixteen, each lane requests 16 rows instead of 4, all of them in flight together)
template <int THREADS>
__global__ void __launch_bounds__(THREADS) vgicp_finalize_rigid_kernel(const FactorDesc* __restrict__ factors, const double* __restrict__ poses,
                                                                       const InlinePoses inl, const double* __restrict__ partials,
                                                                       gp_linearized6* __restrict__ out, const DoneFlags done, const int parts) {
  static_assert(ACC_STRIDE == 32 && (THREADS == 1024 || THREADS == 256), "lane = (slice parity, component); two slices per wave");
  constexpr int kSlices = THREADS / 32, kWaves = THREADS / 64;
  // parts > 1 (synchronous single-factor calls with many tiles): every record entry is LINEAR in the 29 sums, so `parts` workgroups
  // each expand their share of the tiles into a complete record of their own (slot fi * parts + part, own completion word) and the
  // host adds the records in slot order -- the 250 KB of partials of a 1 M-point factor then go through `parts` compute units'
  // L1s instead of one (that was 4.9 of the kernel's 7.1 us)
  // parts < 0: |parts| parts, and a part delivers its 32 SUMS instead of a record: the host adds the parts' sums and expands them
  // (expand_rigid_host) -- the expansion is the same for every part, so it runs once, off the device's critical path
  const bool sums_only = parts < 0;
  const int nparts = sums_only ? -parts : parts;
  const int fi = blockIdx.x / nparts, part = blockIdx.x - fi * nparts;
  const Pose T = inl.use ? load_pose(inl.lin) : load_pose(poses + 16 * (size_t)fi);  // in flight while the partials arrive
  int tile_begin = inl.use ? inl.factor.tile_begin : factors[fi].tile_begin;
  int tile_count = inl.use ? inl.factor.tile_count : factors[fi].tile_count;
  if (nparts > 1) {
    const int per = (tile_count + nparts - 1) / nparts;
    const int lo = min(part * per, tile_count), hi = min(lo + per, tile_count);
    tile_begin += lo;
    tile_count = hi - lo;
  }
  __shared__ double wsum[kWaves][32];
  __shared__ RigidScratch S;
  GP_FIN_TRACE(0);
  if (done.trace && threadIdx.x == 0 && blockIdx.x == 0) done.trace[9] = __builtin_amdgcn_s_getreg(GP_GETREG_XCC_ID);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int comp = threadIdx.x & 31, slice = threadIdx.x >> 5;
  {
    // fixed summation order (deterministic).  All of a lane's rows are requested in ONE batch of up to 32 independent loads
    double total = rigid_slice_total<kSlices, false>(partials + (size_t)tile_begin * ACC_STRIDE + comp, tile_count, slice);
    total += __shfl_xor(total, 32, 64);  // the wave's two slices
    if (lane < 32) wsum[wave][lane] = total;
  }
  GP_FIN_TRACE(1);
  __syncthreads();
  if (wave != 0) return;  // (a finished wave no longer takes part in barriers; none follow anyway)
  if (lane < 32) S.sum[lane] = rigid_wave_tree<kWaves>(&wsum[0][0], lane);
  GP_WAVE_SYNC();
  GP_FIN_TRACE(2);
  if (sums_only) {
    double* out_rec = reinterpret_cast<double*>(out + blockIdx.x);
    if (lane < 32) out_rec[lane] = S.sum[lane];
    GP_FIN_TRACE(3);
    if (done.flags) {
      GP_FIN_TRACE(4);
      __threadfence_system();
      GP_FIN_TRACE(5);
      if (lane == 0) __hip_atomic_store(done.flags + blockIdx.x, done.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      GP_FIN_TRACE(6);
    }
    return;
  }
  rigid_expand_wave(S, T, lane);
  const int t = lane;
  const double* dst = S.dst;
  GP_FIN_TRACE(3);
  // the record leaves in two coalesced sweeps of 8-byte stores (it may be only 8-byte aligned, integrated_vgicp_factor_gpu.cpp:219-220;
  // when `out` is host-mapped memory, scattered stores would each be their own PCIe write)
  double* out_rec = reinterpret_cast<double*>(out + blockIdx.x);
  out_rec[t] = dst[t];
  if (t + 64 < 122) out_rec[t + 64] = dst[t + 64];
  if (done.flags) {
    GP_FIN_TRACE(4);
    __threadfence_system();  // the record is visible to the host before the word that announces it (one wave: no barrier needed)
    GP_FIN_TRACE(5);
    if (t == 0) __hip_atomic_store(done.flags + blockIdx.x, done.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    GP_FIN_TRACE(6);
  }
}

__global__ void __launch_bounds__(kBlockThreads) vgicp_finalize_error_kernel(const FactorDesc* __restrict__ factors, const double* __restrict__ partials,
                                                                             double* __restrict__ out, int single_tile_count, const DoneFlags done) {
  const int fi = blockIdx.x;
  const int tile_begin = single_tile_count >= 0 ? 0 : factors[fi].tile_begin, tile_count = single_tile_count >= 0 ? single_tile_count : factors[fi].tile_count;
  static_assert(kBlockThreads == 256, "error_factor_total is written for 256 threads");
  __shared__ double lds[kBlockThreads / 64];
  const double a = error_factor_total<false>(partials, tile_begin, tile_count, lds);  // (shared with the tile kernel's fused tail: same order, same bits)
  if (threadIdx.x == 0) out[fi] = a;
  signal_done(done, fi, threadIdx.x == 0);
}

// split form of the error finalize for a synchronous single-factor evaluation with >= kFinalizeSplitTiles rows: part g sums rows [g * per, ...) and hands its
// sum to the host, which adds the parts in slot order.  Same code as the fused form runs in the part's last tile workgroup (finalize_part_error).
__global__ void __launch_bounds__(256) vgicp_finalize_error_parts_kernel(const double* __restrict__ partials, const int num_rows, const int rows_per_part, double* __restrict__ out,
                                                                         const int out_stride, const DoneFlags done) {
  __shared__ double wsum[4];
  const int part = blockIdx.x, row_begin = part * rows_per_part;
  finalize_part_error(partials, row_begin, min(rows_per_part, num_rows - row_begin), wsum, out + (size_t)part * out_stride, done.flags + part, done.seq);
}

int wait_done(const unsigned long long* flags_host, size_t count, unsigned long long seq, hipStream_t stream, long spin_us) {
  const volatile unsigned long long* fl = flags_host;
  const auto t0 = std::chrono::steady_clock::now();
  size_t next = 0;
  for (unsigned spins = 1;; spins++) {
    while (next < count && fl[next] == seq) next++;
    if (next == count) {
      std::atomic_thread_fence(std::memory_order_acquire);
      return GP_OK;
    }
    __builtin_ia32_pause();
    // failed kernels, whose words never arrive, are left to the runtime once the spin budget of the call is used up (the caller sizes
    // it on the work: a 100 us budget sent every pass of the 256- and 512-factor batches into hipStreamSynchronize, whose wake-up
    // costs tens of microseconds)
    if ((spins & 255u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us)) break;
  }
  GP_HIP(hipStreamSynchronize(stream));
  return GP_OK;
}

int launch_finalize_single(hipStream_t stream, const double* pose_dev, const double* pose_host, const double* partials, int num_tiles, gp_linearized6* out_dev,
                           bool general, DoneFlags done) {
  InlinePoses inl{};
  memcpy(inl.lin, pose_host, sizeof(double) * 16);
  inl.factor.tile_begin = 0;
  inl.factor.tile_count = num_tiles;
  inl.use = 1;
  if (general)
    hipLaunchKernelGGL(vgicp_finalize_general_kernel, dim3(1), dim3(kFinalizeThreads), 0, stream, (const FactorDesc*)nullptr, inl, partials, out_dev, done);
  else
    hipLaunchKernelGGL(vgicp_finalize_rigid_kernel<kFinalizeThreads>, dim3(1), dim3(kFinalizeThreads), 0, stream, (const FactorDesc*)nullptr, pose_dev, inl, partials, out_dev, done, 1);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? GP_OK : hip_fail(e, "vgicp_finalize_kernel", __FILE__, __LINE__);
}

int launch_finalize_error_single(hipStream_t stream, const double* partials, int num_tiles, double* out_dev, DoneFlags done) {
  hipLaunchKernelGGL(vgicp_finalize_error_kernel, dim3(1), dim3(kBlockThreads), 0, stream, (const FactorDesc*)nullptr, partials, out_dev, num_tiles, done);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? GP_OK : hip_fail(e, "vgicp_finalize_error_kernel", __FILE__, __LINE__);
}

// the same kernels as the two launchers above, one workgroup per factor of a table: rows [tile_begin, tile_begin + tile_count) of factor f, its pose at poses_dev + 16 f,
// its record at out_dev + f (its completion word at done.flags + f).  Same order of sums as the single-factor forms: the same bits.
int launch_finalize_table(hipStream_t stream, const FactorDesc* factors_dev, int num_factors, const double* poses_dev, const double* partials, gp_linearized6* out_dev,
                          bool general, DoneFlags done) {
  InlinePoses inl{};
  inl.use = 0;
  if (general)
    hipLaunchKernelGGL(vgicp_finalize_general_kernel, dim3(num_factors), dim3(kFinalizeThreads), 0, stream, factors_dev, inl, partials, out_dev, done);
  else
    hipLaunchKernelGGL(vgicp_finalize_rigid_kernel<kFinalizeThreads>, dim3(num_factors), dim3(kFinalizeThreads), 0, stream, factors_dev, poses_dev, inl, partials, out_dev, done, 1);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? GP_OK : hip_fail(e, "vgicp_finalize_kernel", __FILE__, __LINE__);
}

int launch_finalize_error_table(hipStream_t stream, const FactorDesc* factors_dev, int num_factors, const double* partials, double* out_dev, DoneFlags done) {
  hipLaunchKernelGGL(vgicp_finalize_error_kernel, dim3(num_factors), dim3(kBlockThreads), 0, stream, factors_dev, partials, out_dev, -1, done);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? GP_OK : hip_fail(e, "vgicp_finalize_error_kernel", __FILE__, __LINE__);
}

// the split form of the error finalize (vgicp_finalize_error_parts_kernel): part g's sum at out_dev + g * out_stride, its completion word at done.flags + g
int launch_finalize_error_parts(hipStream_t stream, const double* partials, int num_rows, int rows_per_part, int parts, double* out_dev, int out_stride, DoneFlags done) {
  hipLaunchKernelGGL(vgicp_finalize_error_parts_kernel, dim3(parts), dim3(256), 0, stream, partials, num_rows, rows_per_part, out_dev, out_stride, done);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? GP_OK : hip_fail(e, "vgicp_finalize_error_parts_kernel", __FILE__, __LINE__);
}

}  // namespace gp

namespace {

// largest |coordinate| over a cloud's finite points, as the bits of a non-negative float (ordered like the unsigned integers they read as)
__global__ void __launch_bounds__(256) source_extent_kernel(const float* __restrict__ points, long long count /* 3 n */, unsigned* __restrict__ out) {
  float m = 0.f;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += 256ll * gridDim.x) {
    const float v = fabsf(points[i]);
    if (v <= 3.402823466e38f) m = fmaxf(m, v);  // (NaN and infinity: no)
  }
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o));
  if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));
}

}  // namespace

namespace gp {

// ... of `count` = 3 n floats, folded into *out (zero before the first launch).  The kernel lives in this unit although only the table build of gp_vgicp_batch.hip uses
// it: it is the unit's one caller of a shuffle at the default width, and without it the optimiser specialises the shuffles of every other kernel here (same
// results, other instructions).
int launch_source_extent(hipStream_t stream, const float* points, long long count, unsigned* out) {
  const int wgs = (int)std::min<long long>(1024, (count + 255) / 256);
  hipLaunchKernelGGL(source_extent_kernel, dim3(wgs), dim3(256), 0, stream, points, count, out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? GP_OK : hip_fail(e, "source_extent_kernel", __FILE__, __LINE__);
}

// ---------------------------------------------------------------------------------------------------------------
// launches of a batch (gp_vgicp_batch.hpp)
// ---------------------------------------------------------------------------------------------------------------

static int grid_tiles(int num_tiles, int xcd_chunk = 0) {
  if (xcd_chunk > 0) {
    const int group = gp::kNumXCD * xcd_chunk;
    return (num_tiles + group - 1) / group * group;
  }
  const int per = (num_tiles + gp::kNumXCD - 1) / gp::kNumXCD;
  return per * gp::kNumXCD;
}


template <int MODE>
int launch_tiles(gp_vgicp_batch* b, const PoseSource& ps, double* partials) {
  if (b->num_tiles <= 0) return GP_OK;
  const int fam = MODE == gp::MODE_LIN_GENERAL ? GP_KERNEL_REFERENCE : b->family;
  // a planned tile list IS the plan: the contiguous map, whatever xcd_chunk says
  // the reference-shaped kernels (the 92-sum path included) keep the contiguous map
  // ... and so does every in-argument launch of the stream kernel (its fixed-tile branch knows no other map)
  const int chunk = (fam == GP_KERNEL_REFERENCE || b->planned || (fam == GP_KERNEL_STREAM && ps.inl.use)) ? 0 : b->tuning.xcd_chunk;
  const dim3 grid_dim(grid_tiles(b->num_tiles, chunk)), block(gp::kBlockThreads);
  const gp::FactorDesc* fd = b->d_factors.as<gp::FactorDesc>();
  const gp::TileDesc* td = b->d_tiles.as<gp::TileDesc>();
  gp::InlinePoses inl = ps.inl;
  inl.stagger = b->tuning.stagger;
  inl.xcd_chunk = chunk;
  inl.tile_points = b->tile_points;
  inl.plan = b->plan;
  inl.trace = b->trace;
  const bool traced = b->trace != nullptr && inl.use && MODE == gp::MODE_LIN;  // the timeline builds exist for single-factor linearise launches
#define GP_ARGS grid_dim, block, 0, b->stream, fd, td, b->num_tiles, ps.d_lin, ps.d_eval, inl, partials
  if constexpr (MODE == gp::MODE_LIN_GENERAL) {
    hipLaunchKernelGGL(gp::vgicp_tile_kernel<MODE>, GP_ARGS);
  } else if (fam == GP_KERNEL_REFERENCE) {
    hipLaunchKernelGGL(gp::vgicp_tile_kernel<MODE>, GP_ARGS);
  } else if (fam == GP_KERNEL_STREAM) {
#define GP_LAUNCH_STREAM(NT, INL, SV, PK, TRACE) hipLaunchKernelGGL((gp::vgicp_stream_kernel<MODE, NT, INL, SV, PK, TRACE>), GP_ARGS)
#define GP_LAUNCH_STREAM_S(INL, SV)                                  \
  do {                                                               \
    if (b->packed) {                                                 \
      if (b->nt) GP_LAUNCH_STREAM(true, INL, SV, true, false);       \
      else GP_LAUNCH_STREAM(false, INL, SV, true, false);            \
    } else {                                                         \
      if (b->nt) GP_LAUNCH_STREAM(true, INL, SV, false, false);      \
      else GP_LAUNCH_STREAM(false, INL, SV, false, false);           \
    }                                                                \
  } while (0)
    if (traced && !b->any_sv) {
      if constexpr (MODE == gp::MODE_LIN) {
        if (b->packed) {
          if (b->nt) GP_LAUNCH_STREAM(true, true, false, true, true);
          else GP_LAUNCH_STREAM(false, true, false, true, true);
        } else {
          if (b->nt) GP_LAUNCH_STREAM(true, true, false, false, true);
          else GP_LAUNCH_STREAM(false, true, false, false, true);
        }
      }
    } else if (inl.use) {
      if (b->any_sv) GP_LAUNCH_STREAM_S(true, true);
      else GP_LAUNCH_STREAM_S(true, false);
    } else {
      if (b->any_sv) GP_LAUNCH_STREAM_S(false, true);
      else GP_LAUNCH_STREAM_S(false, false);
    }
#undef GP_LAUNCH_STREAM_S
#undef GP_LAUNCH_STREAM
  } else {
    // the round-2 family: <MODE, f32 outer products, block grid, lean start, look-ahead lookup>
#define GP_LAUNCH_PIPE(F32, GRID, LEAN, AHEAD) hipLaunchKernelGGL((gp::vgicp_pipeline_kernel<MODE, F32, GRID, LEAN, AHEAD>), GP_ARGS)
    if (fam == GP_KERNEL_HASHED) {
      GP_LAUNCH_PIPE(true, false, false, false);
    } else if (fam == GP_KERNEL_GRID_F64) {
      GP_LAUNCH_PIPE(false, true, false, false);
    } else {  // GP_KERNEL_LOOKAHEAD: 1024-point tiles; the linearise with the look-ahead lookup, the error evaluation without
      if constexpr (MODE == gp::MODE_LIN) GP_LAUNCH_PIPE(true, true, true, true);
      else GP_LAUNCH_PIPE(true, true, true, false);
    }
#undef GP_LAUNCH_PIPE
  }
#undef GP_ARGS
  GP_HIP(hipGetLastError());
  return GP_OK;
}

template int launch_tiles<MODE_LIN>(gp_vgicp_batch*, const PoseSource&, double*);
template int launch_tiles<MODE_ERR>(gp_vgicp_batch*, const PoseSource&, double*);
template int launch_tiles<MODE_LIN_GENERAL>(gp_vgicp_batch*, const PoseSource&, double*);

template <bool GENERAL>
int launch_finalize(gp_vgicp_batch* b, const PoseSource& ps, const double* partials, gp_linearized6* out_dev, gp::DoneFlags done, int parts) {
  if constexpr (GENERAL) {
    hipLaunchKernelGGL(gp::vgicp_finalize_general_kernel, dim3((int)b->factors.size()), dim3(gp::kFinalizeThreads), 0, b->stream, b->d_factors.as<gp::FactorDesc>(), ps.inl,
                       partials, out_dev, done);
  } else {
    const int nparts = parts < 0 ? -parts : parts;  // (parts < 0: the parts deliver their sums, the host expands)
    if (nparts > 1)  // 256-thread parts (1024-thread ones measured slower, round 2)
      hipLaunchKernelGGL(gp::vgicp_finalize_rigid_kernel<256>, dim3((int)b->factors.size() * nparts), dim3(256), 0, b->stream, b->d_factors.as<gp::FactorDesc>(), ps.d_lin,
                         ps.inl, partials, out_dev, done, parts);
    else
      hipLaunchKernelGGL(gp::vgicp_finalize_rigid_kernel<gp::kFinalizeThreads>, dim3((int)b->factors.size() * nparts), dim3(gp::kFinalizeThreads), 0, b->stream,
                         b->d_factors.as<gp::FactorDesc>(), ps.d_lin, ps.inl, partials, out_dev, done, parts);
  }
  GP_HIP(hipGetLastError());
  return GP_OK;
}

template int launch_finalize<false>(gp_vgicp_batch*, const PoseSource&, const double*, gp_linearized6*, DoneFlags, int);
template int launch_finalize<true>(gp_vgicp_batch*, const PoseSource&, const double*, gp_linearized6*, DoneFlags, int);

// device work of one linearisation pass.  rigid == true: 29-sum kernel + adjoint expansion; false: 92-sum kernel
// (exact for any 3x3 block, like the reference's explicit J_s).
int launch_linearize(gp_vgicp_batch* b, const PoseSource& ps, gp_linearized6* out_dev, bool rigid, gp::DoneFlags done, int parts, bool timed) {
  if (b->factors.empty()) return GP_OK;
  double* partials = nullptr;
  GP_TRY(partials_ptr(b, &partials));
  if (timed) GP_HIP(hipEventRecord(b->ev[0], b->stream));
  if (rigid) GP_TRY(launch_tiles<gp::MODE_LIN>(b, ps, partials));
  else GP_TRY(launch_tiles<gp::MODE_LIN_GENERAL>(b, ps, partials));
  if (timed) GP_HIP(hipEventRecord(b->ev[1], b->stream));
  if (rigid) GP_TRY(launch_finalize<false>(b, ps, partials, out_dev, done, parts));
  else GP_TRY(launch_finalize<true>(b, ps, partials, out_dev, done));
  if (timed) GP_HIP(hipEventRecord(b->ev[2], b->stream));
  return GP_OK;
}

int launch_error(gp_vgicp_batch* b, const PoseSource& ps, double* out_dev, gp::DoneFlags done) {
  if (b->factors.empty()) return GP_OK;
  double* partials = nullptr;
  GP_TRY(partials_ptr(b, &partials));
  GP_TRY(launch_tiles<gp::MODE_ERR>(b, ps, partials));
  hipLaunchKernelGGL(gp::vgicp_finalize_error_kernel, dim3((int)b->factors.size()), dim3(gp::kBlockThreads), 0, b->stream, b->d_factors.as<gp::FactorDesc>(),
                     partials, out_dev, -1, done);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

}  // namespace gp
