// gp_registration.hip -- global registration on the device: the occupancy set (FastOccupancyGrid), exact feature matching, RANSAC hypotheses and the closed-form
// alignments.  Device counterparts of ann/fast_occupancy_grid.hpp, registration/impl/ransac_impl.hpp:24-191 and registration/alignment.cpp:11-139; the contract of
// every entry point is in include/gtsam_points_hip.h.  f64 arithmetic on the f32 device points; the arithmetic a host restatement has to reproduce to the bit (cells,
// the polygon error, H) is written without fused multiply-adds: contraction is off for the whole unit and fma() is called where one is wanted.
#pragma clang fp contract(off)

#include <cmath>
#include <cstring>

#include "gp_alignment.hpp"
#include "gp_host.hpp"
#include "gp_occupancy.hpp"

struct gp_occupancy_grid {
  double resolution = 1.0;
  hipStream_t stream = nullptr;
  gp::DeviceArray keys;      // unsigned long long[slots]
  gp::DeviceArray words;     // uint32_t[slots][16]
  gp::DeviceArray counters;  // int[2]: occupied blocks, occupied cells
  uint32_t slots = 0;
  int num_blocks = 0;
  int num_cells = 0;
  ~gp_occupancy_grid() {  // the arrays are pooled blocks that any stream may take next: the work that reads them finishes first
    if (keys.ptr) (void)hipStreamSynchronize(stream);
  }
  gp::OccupancyView view() const {
    gp::OccupancyView v;
    v.keys = keys.as<unsigned long long>();
    v.words = words.as<uint32_t>();
    v.mask = slots - 1;
    v.pad_ = 0;
    v.inv_resolution = 1.0 / resolution;
    return v;
  }
};

namespace gp {

static inline unsigned blocks_for(size_t n, unsigned per_block = 256) { return (unsigned)((n + per_block - 1) / per_block); }

struct Pose16 {
  double m[16];
};
static Pose16 pose_or_identity(const double* pose) {
  Pose16 p;
  for (int i = 0; i < 16; i++) p.m[i] = pose ? pose[i] : (i % 5 == 0 ? 1.0 : 0.0);
  return p;
}

// ---- occupancy set ----------------------------------------------------------------------------------------------------------------------------------------------

// the slot of `key`, claimed if it is new (*claimed = 1); mask + 1 when the table has no room (cannot happen at half load; the caller drops the point)
__device__ __forceinline__ uint32_t occ_find_or_claim(unsigned long long* keys, uint32_t mask, unsigned long long key, int* claimed) {
  uint32_t slot = occ_hash(key) & mask;
  *claimed = 0;
  for (uint32_t probe = 0; probe <= mask; probe++) {
    unsigned long long k = keys[slot];
    if (k == kOccEmpty) {
      k = atomicCAS(&keys[slot], kOccEmpty, key);
      if (k == kOccEmpty) {
        *claimed = 1;
        return slot;
      }
    }
    if (k == key) return slot;
    slot = (slot + 1) & mask;
  }
  return mask + 1;
}

__global__ __launch_bounds__(256) void occupancy_insert_kernel(unsigned long long* keys, uint32_t* words, uint32_t mask, double inv_resolution, const float* __restrict__ points,
                                                               int n, Pose16 pose, int* counters) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const Pose T = load_pose(pose.m);
  int new_block = 0, new_cell = 0;
  if (i < n) {
    unsigned long long key;
    int bit;
    if (occ_cell(T, inv_resolution, points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], key, bit)) {
      const uint32_t slot = occ_find_or_claim(keys, mask, key, &new_block);
      if (slot <= mask) {
        const uint32_t m = 1u << (bit & 31);
        new_cell = (atomicOr(&words[(size_t)slot * 16 + (bit >> 5)], m) & m) == 0;
      }
    }
  }
  const int blocks = wave_sum(new_block), cells = wave_sum(new_cell);
  if ((threadIdx.x & 63) == 0) {
    if (blocks) atomicAdd(&counters[0], blocks);
    if (cells) atomicAdd(&counters[1], cells);
  }
}

// moves every block of a table into a larger one (each key is stored once, so a new slot has one writer)
__global__ __launch_bounds__(256) void occupancy_rehash_kernel(const unsigned long long* __restrict__ old_keys, const uint32_t* __restrict__ old_words, uint32_t old_slots,
                                                               unsigned long long* keys, uint32_t* words, uint32_t mask) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= old_slots) return;
  const unsigned long long key = old_keys[i];
  if (key == kOccEmpty) return;
  int claimed;
  const uint32_t slot = occ_find_or_claim(keys, mask, key, &claimed);
  if (slot > mask) return;
  for (int w = 0; w < 16; w++) atomicOr(&words[(size_t)slot * 16 + w], old_words[(size_t)i * 16 + w]);
}

__global__ __launch_bounds__(256) void occupancy_overlaps_kernel(OccupancyView g, const float* __restrict__ points, int n, Pose16 pose, unsigned char* overlaps, int* count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const Pose T = load_pose(pose.m);
  int hit = 0;
  if (i < n) {
    unsigned long long key;
    int bit;
    if (occ_cell(T, g.inv_resolution, points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], key, bit)) hit = occ_lookup(g, key, bit);
    if (overlaps) overlaps[i] = (unsigned char)hit;
  }
  if (count) {
    const int hits = wave_sum(hit);
    if ((threadIdx.x & 63) == 0 && hits) atomicAdd(count, hits);
  }
}

// The scoring kernel: one workgroup = kScorePoints consecutive points of ONE hypothesis; workgroup b serves list slot b / tiles, tile b % tiles.  The pose is a
// uniform (scalar) load, the cloud (12 B per point) and the table are re-read by every hypothesis from L2 / the infinity cache; the counts are integer atomics,
// one per wave.  list == NULL: hypothesis = slot.  stop: a device flag read first (RANSAC's early stop); num_list: the number of list entries, on the device.
constexpr int kScorePoints = 1024;
__global__ __launch_bounds__(256) void occupancy_overlap_batch_kernel(OccupancyView g, const float* __restrict__ points, int n, const double* __restrict__ poses,
                                                                      const int* __restrict__ list, const int* __restrict__ num_list, int tiles, const int* __restrict__ stop,
                                                                      int* __restrict__ counts) {
  if (stop && *stop) return;
  const int slot = blockIdx.x / tiles, tile = blockIdx.x - slot * tiles;
  if (num_list && slot >= *num_list) return;
  const int h = list ? list[slot] : slot;
  const Pose T = load_pose(poses + 16 * (size_t)h);
  int hits = 0;
#pragma unroll
  for (int k = 0; k < kScorePoints / 256; k++) {
    const int i = tile * kScorePoints + k * 256 + threadIdx.x;
    if (i < n) {
      unsigned long long key;
      int bit;
      if (occ_cell(T, g.inv_resolution, points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], key, bit)) hits += occ_lookup(g, key, bit);
    }
  }
  hits = wave_sum(hits);
  if ((threadIdx.x & 63) == 0 && hits) atomicAdd(&counts[h], hits);
}

static int launch_overlap_batch(const gp_occupancy_grid* grid, const float* points, int n, const double* poses_dev, const int* list, const int* num_list, int num_slots,
                                const int* stop, int* counts, hipStream_t stream) {
  const int tiles = (n + kScorePoints - 1) / kScorePoints;
  if ((long long)tiles * num_slots > 0x7fffffffLL) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_overlap_batch: num_poses x ceil(num_points / 1024) exceeds 2^31 - 1");
  hipLaunchKernelGGL(occupancy_overlap_batch_kernel, dim3((unsigned)(tiles * num_slots)), dim3(256), 0, stream, grid->view(), points, n, poses_dev, list, num_list, tiles, stop,
                     counts);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

static int grid_reserve(gp_occupancy_grid* g, int extra_points) {
  const unsigned long long need = 2ull * ((unsigned long long)g->num_blocks + (unsigned long long)extra_points);
  unsigned long long slots = 64;
  while (slots < need) slots <<= 1;
  if (slots <= g->slots) return GP_OK;
  if (slots > (1ull << 30)) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_insert: the table would exceed 2^30 slots");
  DeviceArray keys, words;
  GP_TRY(keys.alloc_pooled(slots * 8, g->stream));
  GP_TRY(words.alloc_pooled(slots * 64, g->stream));
  GP_HIP(hipMemsetAsync(keys.ptr, 0xff, slots * 8, g->stream));
  GP_HIP(hipMemsetAsync(words.ptr, 0, slots * 64, g->stream));
  if (g->slots && g->num_blocks) {
    hipLaunchKernelGGL(occupancy_rehash_kernel, dim3(blocks_for(g->slots)), dim3(256), 0, g->stream, g->keys.as<unsigned long long>(), g->words.as<uint32_t>(), g->slots,
                       keys.as<unsigned long long>(), words.as<uint32_t>(), (uint32_t)(slots - 1));
    GP_HIP(hipGetLastError());
  }
  if (g->slots) GP_HIP(hipStreamSynchronize(g->stream));  // the old table is freed below
  g->keys.swap(keys);
  g->words.swap(words);
  g->slots = (uint32_t)slots;
  return GP_OK;
}

// wait: read the counts back (one synchronisation); without it the insert is only queued and num_blocks / num_cells stay as they were
static int grid_insert(gp_occupancy_grid* g, const float* points, int n, const double* pose, bool wait = true) {
  if (n == 0) return GP_OK;
  GP_TRY(grid_reserve(g, n));
  hipLaunchKernelGGL(occupancy_insert_kernel, dim3(blocks_for(n)), dim3(256), 0, g->stream, g->keys.as<unsigned long long>(), g->words.as<uint32_t>(), g->slots - 1,
                     1.0 / g->resolution, points, n, pose_or_identity(pose), g->counters.as<int>());
  GP_HIP(hipGetLastError());
  if (!wait) return GP_OK;
  int c[2] = {0, 0};
  GP_HIP(hipMemcpyAsync(c, g->counters.ptr, sizeof(c), hipMemcpyDeviceToHost, g->stream));
  GP_HIP(hipStreamSynchronize(g->stream));
  g->num_blocks = c[0];
  g->num_cells = c[1];
  return GP_OK;
}

static int grid_init(gp_occupancy_grid* g, double resolution, hipStream_t stream, int reserve_points = 0) {
  g->resolution = resolution;
  g->stream = stream;
  GP_TRY(g->counters.alloc_pooled(16, stream));
  GP_HIP(hipMemsetAsync(g->counters.ptr, 0, 16, stream));
  return grid_reserve(g, reserve_points);
}

// ---- feature matching ---------------------------------------------------------------------------------------------------------------------------------------------

// One workgroup = kMatchQueries queries (four per wave), every target row.  The target rows pass through LDS in tiles of 64 (row stride dim | 1 words: the lanes of a
// wave read one column of 64 rows without bank conflicts for any dim); lane t of each wave holds target t of the tile against its wave's four queries, so a target
// element read from LDS serves four sums.  Each lane keeps its best (strict <, ascending index: the lowest index among its ties); the wave's 64 are reduced by
// shuffles, equal distances to the lower index.
constexpr int kMatchQueries = 16;
constexpr int kMatchTile = 64;
__global__ __launch_bounds__(256) void feature_nn_kernel(const float* __restrict__ target, int nt, const float* __restrict__ query, int num_rows, int dim,
                                                         const int* __restrict__ rows, int nq, const int* __restrict__ stop, int* __restrict__ out_index,
                                                         double* __restrict__ out_sq_dist) {
  __shared__ float q_lds[kMatchQueries * GP_FEATURE_MAX_DIM];
  __shared__ float t_lds[kMatchTile * (GP_FEATURE_MAX_DIM + 1)];
  if (stop && *stop) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int stride = dim | 1;
  const int q0 = blockIdx.x * kMatchQueries;
  for (int q = wave; q < kMatchQueries; q += 4) {
    const int qi = q0 + q;
    int row = -1;
    if (qi < nq) row = rows ? rows[qi] : qi;
    if (row >= num_rows) row = -1;
    for (int c = lane; c < dim; c += 64) q_lds[q * GP_FEATURE_MAX_DIM + c] = row >= 0 ? query[(size_t)row * dim + c] : __builtin_nanf("");
  }
  double best[4];
  int best_i[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    best[k] = INFINITY;
    best_i[k] = -1;
  }
  for (int t0 = 0; t0 < nt; t0 += kMatchTile) {
    __syncthreads();  // the queries are in; the previous tile has been read
    const int rows_here = min(kMatchTile, nt - t0);
    for (int r = wave; r < rows_here; r += 4)
      for (int c = lane; c < dim; c += 64) t_lds[r * stride + c] = target[(size_t)(t0 + r) * dim + c];
    __syncthreads();
    if (lane < rows_here) {
      double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
      const float* tr = t_lds + lane * stride;
      const float* qr = q_lds + wave * 4 * GP_FEATURE_MAX_DIM;
      for (int j = 0; j < dim; j++) {
        const double tv = (double)tr[j];
        const double d0 = (double)qr[j] - tv, d1 = (double)qr[GP_FEATURE_MAX_DIM + j] - tv, d2 = (double)qr[2 * GP_FEATURE_MAX_DIM + j] - tv,
                     d3 = (double)qr[3 * GP_FEATURE_MAX_DIM + j] - tv;
        acc0 = fma(d0, d0, acc0);
        acc1 = fma(d1, d1, acc1);
        acc2 = fma(d2, d2, acc2);
        acc3 = fma(d3, d3, acc3);
      }
      const int ti = t0 + lane;
      if (acc0 < best[0]) best[0] = acc0, best_i[0] = ti;
      if (acc1 < best[1]) best[1] = acc1, best_i[1] = ti;
      if (acc2 < best[2]) best[2] = acc2, best_i[2] = ti;
      if (acc3 < best[3]) best[3] = acc3, best_i[3] = ti;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    double d = best[k];
    int bi = best_i[k];
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_xor(d, off);
      const int oi = __shfl_xor(bi, off);
      if (oi >= 0 && (bi < 0 || od < d || (od == d && oi < bi))) d = od, bi = oi;
    }
    const int qi = q0 + wave * 4 + k;
    if (lane == 0 && qi < nq) {
      out_index[qi] = bi;
      out_sq_dist[qi] = bi >= 0 ? d : (double)INFINITY;
    }
  }
}

int launch_feature_nn(const float* target, int nt, const float* query, int num_rows, int dim, const int* rows, int nq, const int* stop, int* out_index, double* out_sq_dist,
                      hipStream_t stream) {  // (declared in gp_alignment.hpp: gp_gnc.hip matches with the same kernel)
  hipLaunchKernelGGL(feature_nn_kernel, dim3(blocks_for(nq, kMatchQueries)), dim3(256), 0, stream, target, nt, query, num_rows, dim, rows, nq, stop, out_index, out_sq_dist);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

// ---- the closed-form alignments (their closed forms and the tree sum: gp_alignment.hpp) ---------------------------------------------------------------------------------

// one edge of the polygon pre-rejection (ransac_impl.hpp:81-83)
__device__ __forceinline__ double poly_edge_error(const Vec3& ta, const Vec3& tb, const Vec3& sa, const Vec3& sb) {
  const double dt = norm3(sub3(ta, tb)), ds = norm3(sub3(sa, sb));
  return fabs(dt - ds) / fmax(fmax(dt, ds), 1e-6);
}

// the weighted N-point alignment in one workgroup: three tree reductions in LDS (fixed order, no floating-point atomics): sum of weights and weighted means, then H
__global__ __launch_bounds__(kAlignThreads) void align_points_kernel(const double* __restrict__ target, const double* __restrict__ source, const double* __restrict__ weights, int n,
                                                                     int dof, double* __restrict__ pose_out) {
  __shared__ double lds[9 * kAlignThreads];
  double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < n; i += kAlignThreads) {
    const double w = weights[i];
    m[0] += w;
    m[1] += w * target[3 * (size_t)i], m[2] += w * target[3 * (size_t)i + 1], m[3] += w * target[3 * (size_t)i + 2];
    m[4] += w * source[3 * (size_t)i], m[5] += w * source[3 * (size_t)i + 1], m[6] += w * source[3 * (size_t)i + 2];
  }
  block_sum(lds, m, 7);
  const Vec3 mt{m[1] / m[0], m[2] / m[0], m[3] / m[0]}, ms{m[4] / m[0], m[5] / m[0], m[6] / m[0]};
  double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < n; i += kAlignThreads) {
    const Vec3 t{target[3 * (size_t)i] - mt.x, target[3 * (size_t)i + 1] - mt.y, target[3 * (size_t)i + 2] - mt.z};
    const Vec3 s{source[3 * (size_t)i] - ms.x, source[3 * (size_t)i + 1] - ms.y, source[3 * (size_t)i + 2] - ms.z};
    add_outer(h, weights[i], t, s);
  }
  block_sum(lds, h, 9);
  if (threadIdx.x == 0) pose_from_H(h, mt, ms, dof, pose_out);
}

// ---- RANSAC -------------------------------------------------------------------------------------------------------------------------------------------------------

struct RansacState {
  int stop;        // set behind the chunk whose scored hypotheses cross the early-stop rate
  int num_list;    // surviving hypotheses of the current chunk
  int best_inliers;
  int best_iteration;
  int num_scored;
  int pad_;
  double best_pose[16];
};

struct RansacArrays {
  int* status;
  int* source_indices;  // [H][3]
  int* target_indices;  // [H][3]
  double* poses;        // [H][16]
  int* inliers;
};

// one thread per iteration of the chunk [begin, begin + count): resets its rows, draws (or takes) the sample, tests the sampled feature rows
__global__ __launch_bounds__(256) void ransac_sample_kernel(RansacState* state, RansacArrays a, int begin, int count, int samples, int num_source, uint64_t seed,
                                                            const int* __restrict__ given, const float* __restrict__ source_features, int dim) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k == 0) state->num_list = 0;
  if (k >= count) return;
  const int it = begin + k;
  int idx[3] = {-1, -1, -1};
  int status = GP_RANSAC_SCORED;
  if (state->stop) {
    status = GP_RANSAC_SKIPPED;
  } else if (given) {
    for (int j = 0; j < samples; j++) idx[j] = given[3 * (size_t)it + j];
  } else {
    unsigned draw = 0;
    int redraws = 0;
    for (int j = 0; j < samples && status == GP_RANSAC_SCORED; j++) {
      for (;;) {
        const int c = (int)ransac_sample_index(seed, (unsigned)it, draw++, (unsigned)num_source);
        if ((j > 0 && c == idx[0]) || (j > 1 && c == idx[1])) {
          if (++redraws > GP_RANSAC_MAX_REDRAWS) {
            status = GP_RANSAC_SAMPLE_FAILED;
            break;
          }
          continue;
        }
        idx[j] = c;
        break;
      }
    }
    if (status != GP_RANSAC_SCORED) idx[0] = idx[1] = idx[2] = -1;
  }
  if (status == GP_RANSAC_SCORED) {
    for (int j = 0; j < samples; j++) {
      const float* f = source_features + (size_t)idx[j] * dim;
      bool zero = true;
      for (int c = 0; c < dim; c++) zero &= fabs((double)f[c]) <= 1e-3;
      if (zero) status = GP_RANSAC_INVALID_FEATURE;
    }
  }
  a.status[it] = status;
  for (int j = 0; j < 3; j++) {
    a.source_indices[3 * (size_t)it + j] = idx[j];
    a.target_indices[3 * (size_t)it + j] = -1;
  }
  for (int j = 0; j < 16; j++) a.poses[16 * (size_t)it + j] = 0.0;
  a.inliers[it] = -1;
}

// the rows the matching kernel searches: the sample of every iteration that is still alive, -1 otherwise
__global__ __launch_bounds__(256) void ransac_rows_kernel(const RansacState* state, RansacArrays a, int begin, int count, int* __restrict__ rows) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= 3 * count) return;
  const int it = begin + k / 3;
  rows[k] = (!state->stop && a.status[it] == GP_RANSAC_SCORED) ? a.source_indices[3 * (size_t)begin + k] : -1;
}

// one thread per iteration: polygon pre-rejection, alignment, taboo list; a survivor joins the chunk's list
__global__ __launch_bounds__(256) void ransac_hypothesis_kernel(RansacState* state, RansacArrays a, int begin, int count, int samples, const float* __restrict__ target, const float* __restrict__ source,
                                                                const int* __restrict__ matched, double poly_error_thresh, const double* __restrict__ taboo_inv, int num_taboo,
                                                                double taboo_rot, double taboo_trans, int* __restrict__ list) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= count || state->stop) return;
  const int it = begin + k;
  if (a.status[it] != GP_RANSAC_SCORED) return;
  const bool three = samples == 3;
  const int* si = a.source_indices + 3 * (size_t)it;
  const int t0i = max(matched[3 * k], 0), t1i = max(matched[3 * k + 1], 0), t2i = three ? max(matched[3 * k + 2], 0) : -1;  // (no match: target 0, ransac_impl.hpp:64)
  a.target_indices[3 * (size_t)it] = t0i, a.target_indices[3 * (size_t)it + 1] = t1i, a.target_indices[3 * (size_t)it + 2] = t2i;
  const Vec3 s0 = point_f64(source, si[0]), s1 = point_f64(source, si[1]), s2 = three ? point_f64(source, si[2]) : Vec3{0, 0, 0};
  const Vec3 t0 = point_f64(target, t0i), t1 = point_f64(target, t1i), t2 = three ? point_f64(target, t2i) : Vec3{0, 0, 0};
  double max_error = poly_edge_error(t0, t1, s0, s1);  // (two samples: both edges are this one)
  if (three) max_error = fmax(max_error, fmax(poly_edge_error(t1, t2, s1, s2), poly_edge_error(t2, t0, s2, s0)));
  if (max_error > poly_error_thresh) {
    a.status[it] = GP_RANSAC_POLY_REJECTED;
    return;
  }
  Vec3 mt, ms;
  if (three) {
    mt = {((t0.x + t1.x) + t2.x) / 3.0, ((t0.y + t1.y) + t2.y) / 3.0, ((t0.z + t1.z) + t2.z) / 3.0};
    ms = {((s0.x + s1.x) + s2.x) / 3.0, ((s0.y + s1.y) + s2.y) / 3.0, ((s0.z + s1.z) + s2.z) / 3.0};
  } else {
    mt = {(t0.x + t1.x) / 2.0, (t0.y + t1.y) / 2.0, (t0.z + t1.z) / 2.0};
    ms = {(s0.x + s1.x) / 2.0, (s0.y + s1.y) / 2.0, (s0.z + s1.z) / 2.0};
  }
  double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  add_outer(h, 1.0, sub3(t0, mt), sub3(s0, ms));
  add_outer(h, 1.0, sub3(t1, mt), sub3(s1, ms));
  if (three) add_outer(h, 1.0, sub3(t2, mt), sub3(s2, ms));
  double pose[16];
  pose_from_H(h, mt, ms, samples == 3 ? 6 : 4, pose);
  for (int j = 0; j < 16; j++) a.poses[16 * (size_t)it + j] = pose[j];
  for (int b = 0; b < num_taboo; b++) {  // delta = taboo^-1 * T (:150)
    const double* q = taboo_inv + 16 * b;
    double d[9];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) d[3 * r + c] = (q[r] * pose[4 * c] + q[4 + r] * pose[4 * c + 1]) + q[8 + r] * pose[4 * c + 2];
    const Vec3 dt{((q[0] * pose[12] + q[4] * pose[13]) + q[8] * pose[14]) + q[12], ((q[1] * pose[12] + q[5] * pose[13]) + q[9] * pose[14]) + q[13],
                  ((q[2] * pose[12] + q[6] * pose[13]) + q[10] * pose[14]) + q[14]};
    const Vec3 v{d[7] - d[5], d[2] - d[6], d[3] - d[1]};  // 2 sin(angle) axis
    const double angle = atan2(norm3(v), ((d[0] + d[4]) + d[8]) - 1.0);
    if (angle < taboo_rot && norm3(dt) < taboo_trans) {
      a.status[it] = GP_RANSAC_TABOO;
      return;
    }
  }
  a.inliers[it] = 0;
  list[atomicAdd(&state->num_list, 1)] = it;
}

// behind the chunk's scoring kernel, one workgroup: the chunk's best scored hypothesis (most inliers, lowest iteration) against the best so far, and the early stop
__global__ __launch_bounds__(256) void ransac_select_kernel(RansacState* state, RansacArrays a, int begin, int count, double stop_above) {
  __shared__ int s_inl[256], s_it[256], s_scored[256], s_stop[256];
  if (state->stop) return;
  int inl = -1, best_it = -1, scored = 0, stop = 0;
  for (int k = threadIdx.x; k < count; k += 256) {
    const int it = begin + k;
    if (a.status[it] != GP_RANSAC_SCORED) continue;
    const int c = a.inliers[it];
    scored++;
    stop |= (double)c > stop_above;
    if (c > inl) inl = c, best_it = it;  // (ascending iteration per thread: strict > keeps the lowest)
  }
  s_inl[threadIdx.x] = inl, s_it[threadIdx.x] = best_it, s_scored[threadIdx.x] = scored, s_stop[threadIdx.x] = stop;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      const int oi = s_inl[threadIdx.x + off], ot = s_it[threadIdx.x + off];
      if (ot >= 0 && (s_it[threadIdx.x] < 0 || oi > s_inl[threadIdx.x] || (oi == s_inl[threadIdx.x] && ot < s_it[threadIdx.x]))) s_inl[threadIdx.x] = oi, s_it[threadIdx.x] = ot;
      s_scored[threadIdx.x] += s_scored[threadIdx.x + off];
      s_stop[threadIdx.x] |= s_stop[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    state->num_scored += s_scored[0];
    if (s_it[0] >= 0 && s_inl[0] > state->best_inliers) {
      state->best_inliers = s_inl[0];
      state->best_iteration = s_it[0];
      for (int j = 0; j < 16; j++) state->best_pose[j] = a.poses[16 * (size_t)s_it[0] + j];
    }
    if (s_stop[0]) state->stop = 1;
  }
}

}  // namespace gp

extern "C" {

int gp_occupancy_grid_create(double resolution, gp_stream_t stream, gp_occupancy_grid_t** out) {
  if (!out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_create: out is NULL");
  *out = nullptr;
  if (!(resolution > 0.0) || !std::isfinite(resolution)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_create: the resolution must be positive and finite");
  auto* g = new gp_occupancy_grid();
  const int rc = gp::grid_init(g, resolution, (hipStream_t)stream);
  if (rc != GP_OK) {
    delete g;
    return rc;
  }
  *out = g;
  return GP_OK;
}

int gp_occupancy_grid_destroy(gp_occupancy_grid_t* grid) {
  delete grid;  // (waits for the grid's stream)
  return GP_OK;
}

int gp_occupancy_grid_insert(gp_occupancy_grid_t* grid, const float* points_dev, int num_points, const double* pose) {
  if (!grid || num_points < 0 || (num_points > 0 && !points_dev)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_insert: bad arguments");
  return gp::grid_insert(grid, points_dev, num_points, pose);
}

int gp_occupancy_grid_overlap(const gp_occupancy_grid_t* grid, const float* points_dev, int num_points, const double* pose, int* num_overlap) {
  if (!grid || !num_overlap || num_points < 0 || (num_points > 0 && !points_dev)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_overlap: bad arguments");
  *num_overlap = 0;
  if (num_points == 0) return GP_OK;
  gp::DeviceArray count;
  GP_TRY(count.alloc_async(16, grid->stream));
  GP_HIP(hipMemsetAsync(count.ptr, 0, 16, grid->stream));
  hipLaunchKernelGGL(gp::occupancy_overlaps_kernel, dim3(gp::blocks_for(num_points)), dim3(256), 0, grid->stream, grid->view(), points_dev, num_points, gp::pose_or_identity(pose),
                     (unsigned char*)nullptr, count.as<int>());
  GP_HIP(hipGetLastError());
  GP_HIP(hipMemcpyAsync(num_overlap, count.ptr, sizeof(int), hipMemcpyDeviceToHost, grid->stream));
  GP_HIP(hipStreamSynchronize(grid->stream));
  return GP_OK;
}

int gp_occupancy_grid_get_overlaps(const gp_occupancy_grid_t* grid, const float* points_dev, int num_points, const double* pose, unsigned char* overlaps_out_dev) {
  if (!grid || num_points < 0 || (num_points > 0 && (!points_dev || !overlaps_out_dev))) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_get_overlaps: bad arguments");
  if (num_points == 0) return GP_OK;
  hipLaunchKernelGGL(gp::occupancy_overlaps_kernel, dim3(gp::blocks_for(num_points)), dim3(256), 0, grid->stream, grid->view(), points_dev, num_points, gp::pose_or_identity(pose),
                     overlaps_out_dev, (int*)nullptr);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

int gp_occupancy_grid_overlap_batch(const gp_occupancy_grid_t* grid, const float* points_dev, int num_points, const double* poses_dev, int num_poses, int* counts_out_dev) {
  if (!grid || num_points < 0 || num_poses < 0 || (num_points > 0 && !points_dev) || (num_poses > 0 && (!poses_dev || !counts_out_dev)))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_overlap_batch: bad arguments");
  if (num_poses == 0) return GP_OK;
  GP_HIP(hipMemsetAsync(counts_out_dev, 0, sizeof(int) * (size_t)num_poses, grid->stream));
  if (num_points == 0) return GP_OK;
  return gp::launch_overlap_batch(grid, points_dev, num_points, poses_dev, nullptr, nullptr, num_poses, nullptr, counts_out_dev, grid->stream);
}

int gp_occupancy_grid_num_occupied_cells(const gp_occupancy_grid_t* grid) { return grid ? grid->num_cells : 0; }

int gp_occupancy_grid_info(const gp_occupancy_grid_t* grid, int* num_slots, int* num_blocks) {
  if (!grid) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_info: grid is NULL");
  if (num_slots) *num_slots = (int)grid->slots;
  if (num_blocks) *num_blocks = grid->num_blocks;
  return GP_OK;
}

int gp_feature_nn_search(const float* target_features_dev, int num_target, const float* query_features_dev, int num_query_rows, int dim, const int* rows_dev, int num_queries,
                         int* indices_out_dev, double* sq_dists_out_dev, gp_stream_t stream) {
  if (dim < 1 || dim > GP_FEATURE_MAX_DIM) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_feature_nn_search: dim must be 1 .. 128");
  if (num_target < 1 || !target_features_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_feature_nn_search: no target features");
  if (num_queries < 0 || num_query_rows < 0 || (num_queries > 0 && (!query_features_dev || !indices_out_dev || !sq_dists_out_dev)))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_feature_nn_search: bad arguments");
  if (!rows_dev && num_queries > num_query_rows) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_feature_nn_search: more queries than query rows");
  if (num_queries == 0) return GP_OK;
  return gp::launch_feature_nn(target_features_dev, num_target, query_features_dev, num_query_rows, dim, rows_dev, num_queries, nullptr, indices_out_dev, sq_dists_out_dev,
                               (hipStream_t)stream);
}

void gp_ransac_params_default(gp_ransac_params* p) {
  if (!p) return;
  p->max_iterations = 5000;
  p->dof = 6;
  p->chunk_iterations = 1024;
  p->num_taboo = 0;
  p->early_stop_inlier_rate = 0.8;
  p->poly_error_thresh = 0.5;
  p->inlier_voxel_resolution = 1.0;
  p->taboo_thresh_rot = 0.5 * M_PI / 180.0;
  p->taboo_thresh_trans = 0.25;
  p->seed = 5489u;
  p->taboo_poses = nullptr;
}

unsigned gp_ransac_sample_index(uint64_t seed, unsigned iteration, unsigned draw, unsigned num_source) { return gp::ransac_sample_index(seed, iteration, draw, num_source); }

int gp_ransac_estimate_pose(const float* target_points_dev, int num_target, const float* source_points_dev, int num_source, const float* target_features_dev,
                            const float* source_features_dev, int dim, const gp_ransac_params* params, const int* sample_indices_dev, const gp_ransac_hypotheses* hypotheses,
                            gp_ransac_result* result, gp_stream_t stream_) {
  using namespace gp;
  if (!params || !result) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: params or result is NULL");
  if (params->dof != 6 && params->dof != 4) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: dof must be 6 or 4");
  const int samples = params->dof == 6 ? 3 : 2;
  if (num_source < samples) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: fewer source points than samples");
  if (num_target < 1) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: the target is empty");
  if (dim < 1 || dim > GP_FEATURE_MAX_DIM) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: dim must be 1 .. 128");
  if (params->num_taboo < 0 || params->num_taboo > GP_RANSAC_MAX_TABOO || (params->num_taboo > 0 && !params->taboo_poses))
    return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: at most 64 taboo poses");
  if (params->max_iterations < 1 || params->chunk_iterations < 1) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: max_iterations and chunk_iterations must be positive");
  if (!(params->inlier_voxel_resolution > 0.0) || !std::isfinite(params->inlier_voxel_resolution))
    return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: the resolution must be positive and finite");
  if (!target_points_dev || !source_points_dev || !target_features_dev || !source_features_dev) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: NULL array");
  hipStream_t stream = (hipStream_t)stream_;
  const int H = params->max_iterations, chunk = std::min(params->chunk_iterations, H);

  // the target's occupancy set (:35-36), sized for the target at once and only queued: the download of the result is the call's one wait
  gp_occupancy_grid grid;
  GP_TRY(grid_init(&grid, params->inlier_voxel_resolution, stream, num_target));
  GP_TRY(grid_insert(&grid, target_points_dev, num_target, nullptr, false));

  DeviceArray own[5], state_d, rows_d, matched_d, dists_d, list_d, taboo_d;
  RansacArrays a;
  const size_t sizes[5] = {sizeof(int) * (size_t)H, sizeof(int) * 3 * (size_t)H, sizeof(int) * 3 * (size_t)H, sizeof(double) * 16 * (size_t)H, sizeof(int) * (size_t)H};
  void* given[5] = {hypotheses ? hypotheses->status : nullptr, hypotheses ? hypotheses->source_indices : nullptr, hypotheses ? hypotheses->target_indices : nullptr,
                    hypotheses ? hypotheses->poses : nullptr, hypotheses ? hypotheses->inliers : nullptr};
  for (int i = 0; i < 5; i++)
    if (!given[i]) {
      GP_TRY(own[i].alloc_async(sizes[i], stream));
      given[i] = own[i].ptr;
    }
  a.status = (int*)given[0], a.source_indices = (int*)given[1], a.target_indices = (int*)given[2], a.poses = (double*)given[3], a.inliers = (int*)given[4];
  GP_TRY(state_d.alloc_async(sizeof(RansacState), stream));
  GP_TRY(rows_d.alloc_async(sizeof(int) * 3 * (size_t)chunk, stream));
  GP_TRY(matched_d.alloc_async(sizeof(int) * 3 * (size_t)chunk, stream));
  GP_TRY(dists_d.alloc_async(sizeof(double) * 3 * (size_t)chunk, stream));
  GP_TRY(list_d.alloc_async(sizeof(int) * (size_t)chunk, stream));
  GP_TRY(taboo_d.alloc_async(sizeof(double) * 16 * (size_t)std::max(params->num_taboo, 1), stream));
  RansacState init;
  std::memset(&init, 0, sizeof(init));
  init.best_inliers = -1;
  init.best_iteration = -1;
  for (int j = 0; j < 16; j += 5) init.best_pose[j] = 1.0;
  GP_HIP(hipMemcpyAsync(state_d.ptr, &init, sizeof(init), hipMemcpyHostToDevice, stream));
  std::vector<double> taboo_inv(16 * (size_t)std::max(params->num_taboo, 1), 0.0);
  for (int b = 0; b < params->num_taboo; b++) {  // Isometry3d::inverse(): R^T, -R^T t
    const double* T = params->taboo_poses + 16 * b;
    double* q = taboo_inv.data() + 16 * b;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) q[4 * c + r] = T[4 * r + c];
    for (int r = 0; r < 3; r++) q[12 + r] = -((q[r] * T[12] + q[4 + r] * T[13]) + q[8 + r] * T[14]);
    q[15] = 1.0;
  }
  if (params->num_taboo) GP_HIP(hipMemcpyAsync(taboo_d.ptr, taboo_inv.data(), sizeof(double) * 16 * params->num_taboo, hipMemcpyHostToDevice, stream));

  RansacState* state = state_d.as<RansacState>();
  const double stop_above = (double)num_source * params->early_stop_inlier_rate;
  for (int begin = 0; begin < H; begin += chunk) {
    const int count = std::min(chunk, H - begin);
    hipLaunchKernelGGL(ransac_sample_kernel, dim3(blocks_for(count)), dim3(256), 0, stream, state, a, begin, count, samples, num_source, params->seed, sample_indices_dev,
                       source_features_dev, dim);
    hipLaunchKernelGGL(ransac_rows_kernel, dim3(blocks_for(3 * (size_t)count)), dim3(256), 0, stream, state, a, begin, count, rows_d.as<int>());
    GP_HIP(hipGetLastError());
    GP_TRY(launch_feature_nn(target_features_dev, num_target, source_features_dev, num_source, dim, rows_d.as<int>(), 3 * count, &state->stop, matched_d.as<int>(),
                             dists_d.as<double>(), stream));
    hipLaunchKernelGGL(ransac_hypothesis_kernel, dim3(blocks_for(count)), dim3(256), 0, stream, state, a, begin, count, samples, target_points_dev, source_points_dev,
                       matched_d.as<int>(), params->poly_error_thresh, taboo_d.as<double>(), params->num_taboo, params->taboo_thresh_rot, params->taboo_thresh_trans,
                       list_d.as<int>());
    GP_HIP(hipGetLastError());
    GP_TRY(launch_overlap_batch(&grid, source_points_dev, num_source, a.poses, list_d.as<int>(), &state->num_list, count, &state->stop, a.inliers, stream));
    hipLaunchKernelGGL(ransac_select_kernel, dim3(1), dim3(256), 0, stream, state, a, begin, count, stop_above);
    GP_HIP(hipGetLastError());
  }
  RansacState fin;
  GP_HIP(hipMemcpyAsync(&fin, state_d.ptr, sizeof(fin), hipMemcpyDeviceToHost, stream));
  GP_HIP(hipStreamSynchronize(stream));
  std::memcpy(result->T_target_source, fin.best_pose, sizeof(fin.best_pose));
  result->best_inliers = std::max(fin.best_inliers, 0);
  result->best_iteration = fin.best_iteration;
  result->num_scored = fin.num_scored;
  result->early_stopped = fin.stop;
  result->inlier_rate = (double)result->best_inliers / (double)num_target;
  return GP_OK;
}

int gp_align_points(const double* target_points_dev, const double* source_points_dev, const double* weights_dev, int num_points, int dof, double* pose_out, gp_stream_t stream_) {
  if (dof != 6 && dof != 4) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_align_points: dof must be 6 or 4");
  if (num_points < 1 || !target_points_dev || !source_points_dev || !weights_dev || !pose_out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_align_points: bad arguments");
  hipStream_t stream = (hipStream_t)stream_;
  gp::DeviceArray pose_d;
  GP_TRY(pose_d.alloc_async(sizeof(double) * 16, stream));
  hipLaunchKernelGGL(gp::align_points_kernel, dim3(1), dim3(gp::kAlignThreads), 0, stream, target_points_dev, source_points_dev, weights_dev, num_points, dof, pose_d.as<double>());
  GP_HIP(hipGetLastError());
  GP_HIP(hipMemcpyAsync(pose_out, pose_d.ptr, sizeof(double) * 16, hipMemcpyDeviceToHost, stream));
  GP_HIP(hipStreamSynchronize(stream));
  return GP_OK;
}

}  // extern "C"
