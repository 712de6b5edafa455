// gp_fpfh.hip -- FPFH descriptors (33-D) on the device over a fixed-radius search: a hashed uniform grid at cell edge search_radius and two kernels, SPFH of every
// point and FPFH of every requested point, one wave per point.  Device counterpart of estimate_fpfh (features/fpfh_estimation.hpp:57-66,
// src/gtsam_points/features/fpfh_estimation.cpp:58-93 and :196-307), CPU-only upstream; the contract of the entry point is in include/gtsam_points_hip.h.
// All arithmetic is f64 on the f32 points and normals, written without fused multiply-adds.
//
// The reference, restated:
//   compute_pair_features(p1, n1, p2, n2) (:58-93)
//     dp = p2 - p1; d = dp.norm(); if (d == 0.0) return Zero                                   (:59-63)
//     ndp = dp / d; angle1 = n1.dot(ndp); angle2 = n2.dot(ndp); alpha = angle1                  (:65-70)
//     if (std::abs(angle1) < std::abs(angle2)) { swap n1, n2; ndp = -ndp; alpha = -angle2; }    (:76-81)
//     v = ndp.cross3(n1).normalized(); if (!v.array().isFinite().all()) return Zero             (:83-86)
//     w = n1.cross3(v); phi = v.dot(n2); theta = atan2(w.dot(n2), n1.dot(n2))                   (:88-91)
//     return (theta, phi, alpha, d)                                                             (:92)
//   normalized() is taken as the division by the norm: a zero cross product (normal parallel to the direction) gives 0 / 0, v is not finite and the pair returns
//   zero -- the case the reference's own finite test is there for.
//   bins (:205-209, :236-238): nf = (f - fmin) * inv_range, fmin = (-pi, -1, -1), inv_range = 1 / (2 pi, 2, 2); bin = clamp(floor(nf * 11), 0, 10).  A NaN feature (a
//   neighbour whose normal is NaN: phi and theta) goes to bin 0, which is what the reference's conversion to int gives on x86-64 behind its max(0).
//   SPFH of point k (:215-247): neighbours = radius_search(p_k, search_radius, max_num_neighbors); size <= 1: zero row; otherwise the three 11-bin integer histograms
//   of the pair features (k, j) over every neighbour j != k (by index), times hist_incr = 100.0 / (size - 1).
//   FPFH of index i (:250-276): size <= 1: zero row; otherwise sum over the neighbours with sq_dist != 0 of spfh[j] * (1.0 / sq_dist), then times
//   100.0 / (sum of the first 11 entries) -- all 33 entries by that one normaliser (the other two are commented out, :272-273).  A row whose first 11 entries sum
//   to zero (a point whose only neighbours are coincident copies of itself) is 0 * inf = NaN, as in the reference.
//   neighbourhood (ann/small_kdtree.hpp:492): every j with d2 = (dx dx + dy dy) + dz dz < search_radius * search_radius, strictly, j = i included.  A point with a
//   non-finite coordinate is nobody's neighbour and its own rows are zero (num_neighbors 0).
//
// THE ONE DEVIATION: which neighbours survive max_num_neighbors.  The reference keeps the first max_num_neighbors in the traversal order of its kd-tree; here the
// grid's cell coordinate is floor(coord / search_radius) in f64 (clamped to +-(2^20 - 3): the clamp never separates true neighbours by more than one cell), the 27
// cells around the query are walked in ascending (dz, dy, dx) order, dx fastest, the points of a cell in ascending original index, and the walk stops after
// max_num_neighbors accepted points.  Both kernels walk by this one rule (fpfh_walk), so they see the same set.  Where the cap does not bind the set is the
// reference's.  num_truncated counts the points whose walk ended at the cap (num_neighbors == max_num_neighbors).
//
// Grid: the points' table slots come from the key table's claim (gp_key_table.hpp: key_claim / key_find on gp_knn_grid.hpp's pack_cell and hash_key; at most n cells
// in >= 2 n slots, so an empty slot always ends a probe, and every probe loop is bounded by the table size besides), the stable radix sort of (slot, index) gives the ascending index inside a cell
// (gp::sort_indices_by_key, gp_cloud_filter.hip: gp_sort.hpp's sort under its retry rule), one kernel gathers points and normals in that order and marks the
// cells' ranges.  The hashed level of gp_knn.hip is not reused: its cell is fast_floor(coord * inv_h) and its scatter leaves the order inside a cell to the atomics.
// Memory: no neighbour lists (N x 10000 does not fit): both kernels re-walk the 27 cells.  Pass 1 leaves 36 ints per point in cell order: 33 counts, the
// neighbour count, two words of padding (nine 16-byte loads per neighbour in pass 2, which forms (double)count * hist_incr itself: the reference's f64 product).
// Determinism: integer histograms (LDS integer atomics); pass 2 sums lane-strided f64 partials in a fixed shuffle tree; no floating-point atomics.
#pragma clang fp contract(off)

#include <cmath>
#include <cstring>

#include "gp_knn_grid.hpp"
#include "gp_select.hpp"

namespace gp {
namespace {

constexpr int kFpfhDim = 33;
constexpr int kFpfhRow = 36;  // ints per point between the passes: 33 counts | num_neighbors | 2 pad
constexpr int kFpfhCellLimit = (1 << 20) - 3;
constexpr int kFpfhWaves = 4;  // points per workgroup

struct FpfhGrid {
  const unsigned long long* keys;  // [mask + 1] packed cell or kEmptyKey
  const int* range;                // [mask + 1][2] first and one-past-last sorted position of the slot's cell
  const float4* points;            // [n] (x, y, z, original index as int bits): cell-major, ascending index inside a cell, non-finite points last
  const float4* normals;           // [n] in the same order
  uint32_t mask;
  int n;
  double radius, r2;
  int cap;
};

__host__ __device__ __forceinline__ int fpfh_cell(double coord, double radius) {
  const double c = floor(coord / radius);
  return c < (double)-kFpfhCellLimit ? -kFpfhCellLimit : (c > (double)kFpfhCellLimit ? kFpfhCellLimit : (int)c);
}

__device__ __forceinline__ bool fpfh_finite(double v) { return fabs(v) < INFINITY; }
__device__ __forceinline__ bool fpfh_finite3(float x, float y, float z) { return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY; }

// slot of every point: its cell's slot in the table, or mask + 1 for a point with a non-finite coordinate (sorts behind every cell)
__global__ __launch_bounds__(256) void fpfh_insert_kernel(const float* __restrict__ points, int n, double radius, unsigned long long* __restrict__ keys, uint32_t mask,
                                                          unsigned* __restrict__ slot_of) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  unsigned slot = mask + 1u;
  if (fpfh_finite3(x, y, z)) {
    const unsigned long long key = pack_cell(fpfh_cell((double)x, radius), fpfh_cell((double)y, radius), fpfh_cell((double)z, radius));
    int claimed;
    slot = key_claim(keys, mask, hash_key(key) & mask, key, &claimed);  // (mask + 1 without room: the same "no cell")
  }
  slot_of[i] = slot;
}

// points and normals in sorted order, every point's sorted position, every cell's range
__global__ __launch_bounds__(256) void fpfh_gather_kernel(const float* __restrict__ points, const float* __restrict__ normals, const unsigned* __restrict__ sorted_slot,
                                                          const int* __restrict__ order, int n, unsigned slots, float4* __restrict__ sorted_points,
                                                          float4* __restrict__ sorted_normals, int* __restrict__ range, int* __restrict__ pos_of) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const size_t i = (size_t)order[j];
  sorted_points[j] = make_float4(points[3 * i], points[3 * i + 1], points[3 * i + 2], __int_as_float((int)i));
  sorted_normals[j] = make_float4(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], 0.0f);
  pos_of[i] = j;
  const unsigned slot = sorted_slot[j];
  if (slot >= slots) return;
  if (j == 0 || sorted_slot[j - 1] != slot) range[2 * (size_t)slot] = j;
  if (j == n - 1 || sorted_slot[j + 1] != slot) range[2 * (size_t)slot + 1] = j + 1;
}

__device__ __forceinline__ int fpfh_find(const FpfhGrid& g, unsigned long long key) { return key_find(g.keys, g.mask, hash_key(key) & g.mask, key); }

// THE walk of both passes, one wave per query: the 27 cells in ascending (dz, dy, dx), 64 candidates of a cell at a time in ascending position (= original index),
// visit(j, point j, d2) in the lanes whose candidate is accepted; at most g.cap accepted points, the lowest lanes first.  Returns the number accepted (wave-uniform).
template <class Visit>
__device__ __forceinline__ int fpfh_walk(const FpfhGrid& g, const float4 q, int lane, Visit&& visit) {
  const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;
  const int cx = fpfh_cell(qx, g.radius), cy = fpfh_cell(qy, g.radius), cz = fpfh_cell(qz, g.radius);
  const unsigned long long below = (1ull << lane) - 1ull;
  int accepted = 0;
  for (int c = 0; c < 27 && accepted < g.cap; c++) {
    const int slot = __builtin_amdgcn_readfirstlane(fpfh_find(g, pack_cell(cx + c % 3 - 1, cy + (c / 3) % 3 - 1, cz + c / 9 - 1)));
    if (slot < 0) continue;
    const int begin = __builtin_amdgcn_readfirstlane(g.range[2 * (size_t)slot]), end = __builtin_amdgcn_readfirstlane(g.range[2 * (size_t)slot + 1]);
    for (int base = begin; base < end && accepted < g.cap; base += 64) {
      const int j = base + lane;
      float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      double d2 = 0.0;
      bool in = false;
      if (j < end) {
        p = g.points[j];
        const double dx = (double)p.x - qx, dy = (double)p.y - qy, dz = (double)p.z - qz;
        d2 = (dx * dx + dy * dy) + dz * dz;
        in = d2 < g.r2;
      }
      const unsigned long long m = __ballot(in);
      const int room = g.cap - accepted;
      if (in && __popcll(m & below) < room) visit(j, p, d2);
      accepted += min(__popcll(m), room);
    }
  }
  return accepted;
}

__device__ __forceinline__ int fpfh_bin(double f, double fmin, double inv_range) {
  const double x = ((f - fmin) * inv_range) * 11.0;
  return !(x >= 0.0) ? 0 : (x >= 10.0 ? 10 : (int)floor(x));  // (NaN: bin 0)
}

// compute_pair_features (:58-93) and the three bins (:236-238), as histogram positions: theta | 11 + phi << 8 | 22 + alpha << 16
__device__ __forceinline__ int fpfh_pair_bins(const float4 p1, const float4 n1, const float4 p2, const float4 n2) {
  double theta = 0.0, phi = 0.0, alpha = 0.0;
  const double dpx = (double)p2.x - (double)p1.x, dpy = (double)p2.y - (double)p1.y, dpz = (double)p2.z - (double)p1.z;
  const double d = sqrt((dpx * dpx + dpy * dpy) + dpz * dpz);
  if (d != 0.0) {
    double ux = dpx / d, uy = dpy / d, uz = dpz / d;
    double mx = (double)n1.x, my = (double)n1.y, mz = (double)n1.z, ox = (double)n2.x, oy = (double)n2.y, oz = (double)n2.z;
    const double angle1 = (mx * ux + my * uy) + mz * uz, angle2 = (ox * ux + oy * uy) + oz * uz;
    double a = angle1;
    if (fabs(angle1) < fabs(angle2)) {
      double t;
      t = mx, mx = ox, ox = t;
      t = my, my = oy, oy = t;
      t = mz, mz = oz, oz = t;
      ux = -ux, uy = -uy, uz = -uz;
      a = -angle2;
    }
    double vx = uy * mz - uz * my, vy = uz * mx - ux * mz, vz = ux * my - uy * mx;
    const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
    vx /= vn, vy /= vn, vz /= vn;
    if (fpfh_finite(vx) && fpfh_finite(vy) && fpfh_finite(vz)) {
      const double wx = my * vz - mz * vy, wy = mz * vx - mx * vz, wz = mx * vy - my * vx;
      phi = (vx * ox + vy * oy) + vz * oz;
      theta = atan2((wx * ox + wy * oy) + wz * oz, (mx * ox + my * oy) + mz * oz);
      alpha = a;
    }
  }
  return fpfh_bin(theta, -M_PI, 1.0 / (M_PI + M_PI)) | (11 + fpfh_bin(phi, -1.0, 0.5)) << 8 | (22 + fpfh_bin(alpha, -1.0, 0.5)) << 16;
}

// pass 1: the wave of sorted position q leaves rows[q] = 33 counts | num_neighbors, and the caller's SPFH row and neighbour count at the point's original index
__global__ __launch_bounds__(64 * kFpfhWaves) void fpfh_spfh_kernel(const FpfhGrid g, int* __restrict__ rows, double* __restrict__ spfh_out, int* __restrict__ num_neighbors_out,
                                                                    int* __restrict__ num_truncated) {
  __shared__ int hist[kFpfhWaves][kFpfhRow];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * kFpfhWaves + wave;
  if (lane < kFpfhRow) hist[wave][lane] = 0;
  __syncthreads();
  int count = 0, self = -1;
  if (q < g.n) {
    const float4 pq = g.points[q];
    self = __float_as_int(pq.w);
    if (fpfh_finite3(pq.x, pq.y, pq.z)) {
      const float4 nq = g.normals[q];
      int* h = hist[wave];
      count = fpfh_walk(g, pq, lane, [&](int j, const float4 pj, double) {
        if (__float_as_int(pj.w) == self) return;
        const int b = fpfh_pair_bins(pq, nq, pj, g.normals[j]);
        atomicAdd(h + (b & 255), 1);
        atomicAdd(h + ((b >> 8) & 255), 1);
        atomicAdd(h + (b >> 16), 1);
      });
    }
  }
  __syncthreads();
  if (q >= g.n) return;
  if (lane < kFpfhRow) {
    const int c = (lane < kFpfhDim && count > 1) ? hist[wave][lane] : 0;
    rows[(size_t)q * kFpfhRow + lane] = lane == kFpfhDim ? count : c;
    if (spfh_out && lane < kFpfhDim) spfh_out[(size_t)self * kFpfhDim + lane] = count > 1 ? (double)c * (100.0 / (double)(count - 1)) : 0.0;
  }
  if (lane == 0) {
    if (num_neighbors_out) num_neighbors_out[self] = count;
    if (count == g.cap) atomicAdd(num_truncated, 1);
  }
}

// pass 2: request k (index indices[k], or the point at sorted position k when indices is null) -> its FPFH row (row k, or the point's original index)
__global__ __launch_bounds__(64 * kFpfhWaves) void fpfh_fpfh_kernel(const FpfhGrid g, const int* __restrict__ rows, const int* __restrict__ pos_of, const int* __restrict__ indices,
                                                                    int m, double* __restrict__ out, float* __restrict__ out_f32) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * kFpfhWaves + (threadIdx.x >> 6);
  if (k >= m) return;
  const int q = indices ? pos_of[indices[k]] : k;
  const float4 pq = g.points[q];
  const size_t row = indices ? (size_t)k : (size_t)__float_as_int(pq.w);
  const int n_q = rows[(size_t)q * kFpfhRow + kFpfhDim];
  double value = 0.0;
  if (n_q > 1) {
    double acc[kFpfhDim];
#pragma unroll
    for (int b = 0; b < kFpfhDim; b++) acc[b] = 0.0;
    fpfh_walk(g, pq, lane, [&](int j, const float4, double d2) {
      if (d2 == 0.0) return;
      const int4* r = reinterpret_cast<const int4*>(rows + (size_t)j * kFpfhRow);
      int c[kFpfhRow];
#pragma unroll
      for (int v = 0; v < kFpfhRow / 4; v++) {
        const int4 x = r[v];
        c[4 * v] = x.x, c[4 * v + 1] = x.y, c[4 * v + 2] = x.z, c[4 * v + 3] = x.w;
      }
      if (c[kFpfhDim] <= 1) return;  // (a zero SPFH row)
      const double hist_incr = 100.0 / (double)(c[kFpfhDim] - 1), weight = 1.0 / d2;
#pragma unroll
      for (int b = 0; b < kFpfhDim; b++) acc[b] += ((double)c[b] * hist_incr) * weight;
    });
    // the lanes' partials in a fixed tree; every lane ends with every sum
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int b = 0; b < kFpfhDim; b++) acc[b] += __shfl_xor(acc[b], off, 64);
    double first = acc[0];
#pragma unroll
    for (int b = 1; b < 11; b++) first += acc[b];
    const double norm1 = 100.0 / first;
#pragma unroll
    for (int b = 0; b < kFpfhDim; b++) value = lane == b ? acc[b] * norm1 : value;
  }
  if (lane < kFpfhDim) {
    if (out) out[row * kFpfhDim + lane] = value;
    if (out_f32) out_f32[row * kFpfhDim + lane] = (float)value;
  }
}

uint32_t fpfh_slots(int n) {
  uint32_t slots = 1024;
  while (slots < 2u * (uint32_t)n) slots <<= 1;  // at most n cells: load factor <= 0.5, an empty slot always exists
  return slots;
}

// measurement (gp_debug_fpfh_phase_times): the stream's time of the grid build, pass 1 and pass 2 of this thread's last call
thread_local bool g_fpfh_timing = false;
thread_local double g_fpfh_ms[3] = {0.0, 0.0, 0.0};
struct FpfhEvents {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  bool on = false;
  int mark(int k, hipStream_t s) {
    if (!on) return GP_OK;
    if (!e[k]) GP_HIP(hipEventCreate(&e[k]));
    GP_HIP(hipEventRecord(e[k], s));
    return GP_OK;
  }
  void read() {
    for (int k = 0; k < 3; k++) {
      float ms = 0.0f;
      g_fpfh_ms[k] = (on && e[k] && e[k + 1] && hipEventElapsedTime(&ms, e[k], e[k + 1]) == hipSuccess) ? (double)ms : 0.0;
    }
  }
  ~FpfhEvents() {
    for (hipEvent_t ev : e)
      if (ev) (void)hipEventDestroy(ev);
  }
};

struct FpfhArrays {
  DeviceArray keys, range, points, normals, pos_of;
  void release_on(hipStream_t s) { keys.release_on(s), range.release_on(s), points.release_on(s), normals.release_on(s), pos_of.release_on(s); }
};

// the grid of one call: insert, sort by slot (gp_cloud_filter.hip: the sort's kernels stay out of this unit's resource remarks), gather
int fpfh_build(const float* points, const float* normals, int n, double radius, uint32_t slots, FpfhArrays& a, hipStream_t s, const char* who) {
  int key_bits = 1;  // values 0 .. slots
  while ((slots >> key_bits) != 0u) key_bits++;
  DeviceArray slot_of, sorted_slot, order;
  GP_TRY(slot_of.alloc_async(sizeof(unsigned) * (size_t)n, s));
  GP_TRY(sorted_slot.alloc_async(sizeof(unsigned) * (size_t)n, s));
  GP_TRY(order.alloc_async(sizeof(int) * (size_t)n, s));
  GP_HIP(hipMemsetAsync(a.keys.ptr, 0xff, sizeof(unsigned long long) * slots, s));
  hipLaunchKernelGGL(fpfh_insert_kernel, dim3(blocks_of((size_t)n)), dim3(256), 0, s, points, n, radius, a.keys.as<unsigned long long>(), slots - 1u, slot_of.as<unsigned>());
  GP_HIP(hipGetLastError());
  GP_TRY(sort_indices_by_key(slot_of.as<unsigned>(), n, key_bits, sorted_slot.as<unsigned>(), order.as<int>(), s, who));  // (waits)
  hipLaunchKernelGGL(fpfh_gather_kernel, dim3(blocks_of((size_t)n)), dim3(256), 0, s, points, normals, (const unsigned*)sorted_slot.as<unsigned>(), (const int*)order.as<int>(), n, slots,
                     a.points.as<float4>(), a.normals.as<float4>(), a.range.as<int>(), a.pos_of.as<int>());
  GP_HIP(hipGetLastError());
  slot_of.release_on(s), sorted_slot.release_on(s), order.release_on(s);
  return GP_OK;
}

}  // namespace
}  // namespace gp

extern "C" {

void gp_fpfh_params_default(gp_fpfh_params* p) {
  if (!p) return;
  p->search_radius = 5.0;  // features/fpfh_estimation.hpp:60-64
  p->max_num_neighbors = 10000;
}

int gp_debug_fpfh_phase_times(int enable, double* ms_out) {
  gp::g_fpfh_timing = enable != 0;
  if (ms_out) std::memcpy(ms_out, gp::g_fpfh_ms, sizeof(gp::g_fpfh_ms));
  return GP_OK;
}

int gp_estimate_fpfh(const float* points_dev, const float* normals_dev, int n, const gp_fpfh_params* params, const int* indices_dev, int num_indices, double* fpfh_out_dev,
                     float* fpfh_out_f32_dev, double* spfh_out_dev, int* num_neighbors_out_dev, int* num_truncated_out, gp_stream_t stream) {
  using namespace gp;
  const std::string who = "gp_estimate_fpfh";
  if (!params) return fail(GP_ERROR_INVALID_ARGUMENT, who + ": params is NULL");
  if (!points_dev || !normals_dev) return fail(GP_ERROR_INVALID_ARGUMENT, who + ": points or normals is NULL");
  if (n < 1) return fail(GP_ERROR_INVALID_ARGUMENT, who + ": n must be positive");
  if (n >= (1 << 30)) return fail(GP_ERROR_INVALID_ARGUMENT, who + ": n must be below 2^30");
  if (!(params->search_radius > 0.0) || !std::isfinite(params->search_radius)) return fail(GP_ERROR_INVALID_ARGUMENT, who + ": search_radius must be finite and positive");
  if (params->max_num_neighbors < 1) return fail(GP_ERROR_INVALID_ARGUMENT, who + ": max_num_neighbors must be positive");
  if (num_indices < 0) return fail(GP_ERROR_INVALID_ARGUMENT, who + ": num_indices is negative");
  const bool want_fpfh = fpfh_out_dev || fpfh_out_f32_dev;
  if (!want_fpfh && !spfh_out_dev) return fail(GP_ERROR_INVALID_ARGUMENT, who + ": no output: fpfh_out_dev, fpfh_out_f32_dev and spfh_out_dev are all NULL");
  hipStream_t s = (hipStream_t)stream;
  const uint32_t slots = fpfh_slots(n);
  FpfhEvents ev;
  ev.on = g_fpfh_timing;
  FpfhArrays a;
  DeviceArray rows, truncated;
  GP_TRY(a.keys.alloc_async(sizeof(unsigned long long) * slots, s));
  GP_TRY(a.range.alloc_async(sizeof(int) * 2 * (size_t)slots, s));
  GP_TRY(a.points.alloc_async(sizeof(float4) * (size_t)n, s));
  GP_TRY(a.normals.alloc_async(sizeof(float4) * (size_t)n, s));
  GP_TRY(a.pos_of.alloc_async(sizeof(int) * (size_t)n, s));
  GP_TRY(rows.alloc_async(sizeof(int) * kFpfhRow * (size_t)n, s));
  GP_TRY(truncated.alloc_async(sizeof(int), s));
  GP_TRY(ev.mark(0, s));
  GP_TRY(fpfh_build(points_dev, normals_dev, n, params->search_radius, slots, a, s, who.c_str()));
  GP_TRY(ev.mark(1, s));
  FpfhGrid g;
  g.keys = a.keys.as<unsigned long long>();
  g.range = a.range.as<int>();
  g.points = a.points.as<float4>();
  g.normals = a.normals.as<float4>();
  g.mask = slots - 1u;
  g.n = n;
  g.radius = params->search_radius;
  g.r2 = params->search_radius * params->search_radius;
  g.cap = params->max_num_neighbors;
  GP_HIP(hipMemsetAsync(truncated.ptr, 0, sizeof(int), s));
  const unsigned point_blocks = (unsigned)(((size_t)n + kFpfhWaves - 1) / kFpfhWaves);
  hipLaunchKernelGGL(fpfh_spfh_kernel, dim3(point_blocks), dim3(64 * kFpfhWaves), 0, s, g, rows.as<int>(), spfh_out_dev, num_neighbors_out_dev, truncated.as<int>());
  GP_HIP(hipGetLastError());
  GP_TRY(ev.mark(2, s));
  const int m = indices_dev ? num_indices : n;
  if (want_fpfh && m > 0) {
    hipLaunchKernelGGL(fpfh_fpfh_kernel, dim3((unsigned)(((size_t)m + kFpfhWaves - 1) / kFpfhWaves)), dim3(64 * kFpfhWaves), 0, s, g, (const int*)rows.as<int>(),
                       (const int*)a.pos_of.as<int>(), indices_dev, m, fpfh_out_dev, fpfh_out_f32_dev);
    GP_HIP(hipGetLastError());
  }
  GP_TRY(ev.mark(3, s));
  int cut = 0;
  GP_HIP(hipMemcpyAsync(&cut, truncated.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));  // (the outputs are the caller's to read, on any stream)
  if (num_truncated_out) *num_truncated_out = cut;
  ev.read();
  a.release_on(s), rows.release_on(s), truncated.release_on(s);
  return GP_OK;
}

}  // extern "C"
