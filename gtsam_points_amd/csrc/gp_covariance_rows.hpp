// gp_covariance_rows.hpp -- the row-tiled first pass of the covariance estimator (GP_TUNE_KNN_STRUCTURE = 3, an experiment kept with its tests): one wave per
// occupied cell row scans the rows around it through LDS (covariance_rows_kernel), a second kernel settles the queries whose k nearest are provably among what was
// kept (covariance_settle_kernel) and lists the rest for the per-lane search.  A part of gp_covariance.hip.
//
// Replaces (reference, CPU only): the k-NN loop of features/covariance_estimation.cpp:18-53 for the queries it settles.
#pragma once

#include "gp_covariance_point.hpp"

namespace gp {

// estimate_covariances, tiled: ONE WAVE PER OCCUPIED CELL ROW (the <= 4 x-adjacent cells of one (y, z) row of a block).  The queries
// are the row's own points -- one contiguous range of the cell-sorted array, ~20-70 of them -- and the candidates are the points of the
// cells x_min-1 .. x_max+1 of the 3 x 3 rows around it: 27 (block, row, x-mask) pieces, each again ONE contiguous range because
// occupied cells of a row have consecutive ordinals.  The 27 lookups run on 27 lanes at once (one latency chain for the whole row
// instead of one per lane and cell), the candidates are staged through LDS with coalesced loads and scanned by every query lane with
// broadcast reads: no per-lane pointer chasing, no divergence in the scan loop, and only ~1.5x the candidates a single query needs
// (the block-sized tiles tried first scanned 15-30x: DESIGN.md section 4.8).  A query is settled when its k-th distance is no
// larger than its distance to the border of that region (>= one cell edge): every point outside is farther.  Anything else -- sparse
// neighbourhoods, rows too dense for one wave -- is appended to `todo_list` and goes through the per-lane search, so the result is
// exact either way.
constexpr int kRowThreads = 64;       // one wave per workgroup: __syncthreads() is free and rows finish independently
constexpr int kRowCand = 256;         // candidates per LDS chunk (4 KB)
constexpr int kRowMaxCand = 8192;     // denser neighbourhoods (near field) are left to the per-lane search
constexpr int kRowMaxQueries = 512;
constexpr int kTileQueue = 32;        // per-lane queue of candidates that passed the f32 filter (2 B each)
constexpr int kTileKeep = 12;         // f32 top list: k (<= 10) + 2 entries of slack for the exactness check

// f32 top list of the tiled kernel: same insertion rule as TopK, floats, compile-time indices only
struct TopF {
  float d[kTileKeep];
  int idx[kTileKeep];
  __device__ void init() {
#pragma unroll
    for (int j = 0; j < kTileKeep; j++) {
      d[j] = __builtin_inff();
      idx[j] = -1;
    }
  }
  __device__ float bound() const { return d[kTileKeep - 1]; }
  __device__ void push(int index, float dist) {
    if (!(dist < d[kTileKeep - 1])) return;
    bool placed = false;
#pragma unroll
    for (int j = kTileKeep - 1; j >= 0; j--) {
      if (!placed) {
        if (j > 0 && dist < d[j - 1]) {
          d[j] = d[j - 1];
          idx[j] = idx[j - 1];
        } else {
          d[j] = dist;
          idx[j] = index;
          placed = true;
        }
      }
    }
  }
};

// appends the sorted positions of the lanes with `flag` to todo_list (one atomic per wave; the order of the list does not matter:
// every leftover query writes its own output slot)
__device__ __forceinline__ void todo_append(bool flag, int pos, int* __restrict__ todo_list, int* __restrict__ todo_count) {
  const unsigned long long m = __ballot(flag);
  if (m == 0ull) return;
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == __ffsll((long long)m) - 1) base = atomicAdd(todo_count, __popcll(m));
  base = __shfl(base, __ffsll((long long)m) - 1, 64);
  if (flag) todo_list[base + __popcll(m & ((1ull << lane) - 1ull))] = pos;
}

// Scan kernel.  The scan loop is an LDS broadcast read, an f32 distance, a compare and a 2-byte LDS append for the lanes whose
// candidate passes.  What passes is pushed into the lane's f32 top list only when a queue is full or the chunk ends -- then every lane
// is busy with its OWN candidates, instead of the whole wave executing an insertion whenever any one lane has a hit.  The pieces are
// scanned own row first, so the acceptance threshold is tight after the first few dozen candidates.  Per query the kernel leaves the
// kTileKeep nearest candidates by f32 distance (original indices), the kTileKeep-th f32 distance and the query's distance to the
// border of the scanned region; the exact decision is taken by covariance_settle_kernel below with all lanes busy (a row fills a
// quarter of a wave on average, and the f64 work is the expensive part).
struct RowScanOut {
  int* kept;     // [kTileKeep][nq] original indices (-1: none), by sorted position
  float* bound;  // [nq] kTileKeep-th f32 squared distance (inf: fewer candidates than that), < 0: row not scanned
  float* safe;   // [nq] distance to the border of the scanned region, rounded down
  int nq;
};

__global__ void __launch_bounds__(kRowThreads) covariance_rows_kernel(BinGridView g, const int* __restrict__ occ_blocks, RowScanOut out, int knock) {
  __shared__ float4 cand[kRowCand];
  __shared__ unsigned short queue[kTileQueue][kRowThreads];
  __shared__ int rstart[27], rpref[28];
  const int lane = threadIdx.x;
  const int row = blockIdx.x & 15;                  // y + 4 z inside the block
  const long long b = occ_blocks[blockIdx.x >> 4];  // work list: the occupied blocks only (a LiDAR box is >99 % empty blocks)
  const GridBlock me = g.blocks[b];
  const unsigned rowbits = (unsigned)(me.bits >> (4 * row)) & 0xFu;
  if (rowbits == 0u) return;
  const int ord0 = me.base + __popcll(me.bits & ((1ull << (4 * row)) - 1ull));
  const int q0 = g.cell_start[ord0];
  const int Q = g.cell_start[ord0 + __popc(rowbits)] - q0;
  const int dim0 = g.geom.dim[0], dim1 = g.geom.dim[1], dim2 = g.geom.dim[2];
  const int bx = (int)(b % dim0), by = (int)((b / dim0) % dim1), bz = (int)(b / ((long long)dim0 * dim1));
  // cell coordinates relative to the grid's first cell; the candidate region is x in [cx_lo, cx_hi], y in cy +- 1, z in cz +- 1
  const int cy = 4 * by + (row & 3), cz = 4 * bz + (row >> 2);
  const int cx_lo = 4 * bx + (__ffs((int)rowbits) - 1) - 1, cx_hi = 4 * bx + (31 - __clz((int)rowbits)) + 1;
  int len = 0;
  if (lane < 27) {
    // piece order: own row first, then the rows sharing a face with it, then the diagonal ones; own block column first in each
    const int t = lane / 3, u = lane % 3;
    const int dy = (int)((0x22161u >> (2 * t)) & 3u) - 1;  // two bits per entry: t = 0..8 -> dy = 0,-1,1, 0,0, -1,1,-1,1
    const int dz = (int)((0x28215u >> (2 * t)) & 3u) - 1;  //                                    dz = 0, 0,0,-1,1, -1,-1,1,1
    const int nbx = bx + (u == 0 ? 0 : (u == 1 ? -1 : 1)), ny = cy + dy, nz = cz + dz;
    int start = 0;
    const int lo = max(cx_lo - 4 * nbx, 0), hi = min(cx_hi - 4 * nbx, 3);  // cells of block column nbx inside the x-range
    if (lo <= hi && nbx >= 0 && nbx < dim0 && ny >= 0 && ny < 4 * dim1 && nz >= 0 && nz < 4 * dim2) {
      const GridBlock nb = g.blocks[((long long)(nz >> 2) * dim1 + (ny >> 2)) * dim0 + nbx];
      const int sh = 4 * ((ny & 3) + 4 * (nz & 3)) + lo;
      const unsigned m = (unsigned)(nb.bits >> sh) & ((2u << (hi - lo)) - 1u);
      if (m) {
        const int o = nb.base + __popcll(nb.bits & ((1ull << sh) - 1ull));
        start = g.cell_start[o];
        len = g.cell_start[o + __popc(m)] - start;
      }
    }
    rstart[lane] = start;
  }
  int incl = len;  // inclusive prefix of the 27 piece lengths across the lanes
#pragma unroll
  for (int off = 1; off < 32; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane < 27) rpref[lane + 1] = incl;
  if (lane == 0) rpref[0] = 0;
  __syncthreads();
  const int C = rpref[27];
  if (knock == 1) return;
  if (Q > kRowMaxQueries || C > kRowMaxCand) {
    for (int t = lane; t < Q; t += kRowThreads) out.bound[q0 + t] = -1.0f;
    return;
  }
  // the region's faces (metres)
  const double rlo[3] = {(double)(4 * g.geom.lo[0] + cx_lo) * g.h, (double)(4 * g.geom.lo[1] + cy - 1) * g.h, (double)(4 * g.geom.lo[2] + cz - 1) * g.h};
  const double rhi[3] = {(double)(4 * g.geom.lo[0] + cx_hi + 1) * g.h, (double)(4 * g.geom.lo[1] + cy + 2) * g.h, (double)(4 * g.geom.lo[2] + cz + 2) * g.h};
  for (int pass = 0; pass * kRowThreads < Q; pass++) {
    const int qi = pass * kRowThreads + lane;
    const bool active = qi < Q;
    const float4 self = g.sorted[q0 + (active ? qi : 0)];
    TopF top;
    top.init();
    int queued = 0;
    auto drain = [&]() {  // every lane inserts its own queued candidates (f32 distance recomputed from LDS)
      for (int i = 0; __any(i < queued); i++) {
        if (i < queued) {
          const float4 v = cand[queue[i][lane]];
          const float dxf = v.x - self.x, dyf = v.y - self.y, dzf = v.z - self.z;
          top.push(__float_as_int(v.w), dxf * dxf + dyf * dyf + dzf * dzf);
        }
      }
      queued = 0;
    };
    for (int c0 = 0; c0 < C; c0 += kRowCand) {
      __syncthreads();  // the previous chunk has been consumed
      const int cnt = min(kRowCand, C - c0);
      for (int i = lane; i < cnt; i += kRowThreads) {
        const int gi = c0 + i;
        int r = 0;
#pragma unroll
        for (int t = 1; t < 27; t++) r += (rpref[t] <= gi) ? 1 : 0;  // piece holding candidate gi (prefix sums are non-decreasing)
        cand[i] = g.sorted[rstart[r] + (gi - rpref[r])];
      }
      __syncthreads();
      if (knock == 2) continue;
      float thr = top.bound();
      // four candidates per step: the four broadcast reads are in flight together, one queue-full test per step
      const int cnt4 = cnt & ~3;
      for (int j = 0; j < cnt4; j += 4) {
        const float4 v0 = cand[j], v1 = cand[j + 1], v2 = cand[j + 2], v3 = cand[j + 3];
        const float ax = v0.x - self.x, ay = v0.y - self.y, az = v0.z - self.z;
        const float bx_ = v1.x - self.x, by_ = v1.y - self.y, bz_ = v1.z - self.z;
        const float cx_ = v2.x - self.x, cy_ = v2.y - self.y, cz_ = v2.z - self.z;
        const float dx_ = v3.x - self.x, dy_ = v3.y - self.y, dz_ = v3.z - self.z;
        const float d0 = ax * ax + ay * ay + az * az, d1 = bx_ * bx_ + by_ * by_ + bz_ * bz_;
        const float d2 = cx_ * cx_ + cy_ * cy_ + cz_ * cz_, d3 = dx_ * dx_ + dy_ * dy_ + dz_ * dz_;
        if (active) {
          if (d0 < thr) queue[queued++][lane] = (unsigned short)j;
          if (d1 < thr) queue[queued++][lane] = (unsigned short)(j + 1);
          if (d2 < thr) queue[queued++][lane] = (unsigned short)(j + 2);
          if (d3 < thr) queue[queued++][lane] = (unsigned short)(j + 3);
        }
        if (__any(queued > kTileQueue - 4)) {
          if (knock == 3) queued = 0;
          drain();
          thr = top.bound();
        }
      }
      for (int j = cnt4; j < cnt; j++) {
        const float4 v = cand[j];
        const float dxf = v.x - self.x, dyf = v.y - self.y, dzf = v.z - self.z;
        if (active && dxf * dxf + dyf * dyf + dzf * dzf < thr) queue[queued++][lane] = (unsigned short)j;
      }
      drain();  // the chunk is about to be replaced (at most kTileQueue - 4 + 3 entries are queued)
    }
    if (active) {
      const size_t pos = (size_t)q0 + qi;
#pragma unroll
      for (int j = 0; j < kTileKeep; j++) out.kept[(size_t)j * out.nq + pos] = top.idx[j];
      out.bound[pos] = top.bound();
      double safe = 1.0e300;
      const double q[3] = {(double)self.x, (double)self.y, (double)self.z};
#pragma unroll
      for (int a = 0; a < 3; a++) safe = fmin(safe, fmin(q[a] - rlo[a], rhi[a] - q[a]));
      out.safe[pos] = (float)fmax(safe, 0.0) * 0.999999f;
    }
  }
}

// Decision kernel, one query per lane in sorted order: exact re-score of the kept candidates in f64 (the reference compares doubles),
// in f32 rank order.  A query is settled only if (i) the k-th exact distance is below the kTileKeep-th f32 distance by more than f32
// rounding -- everything that was filtered out has an f32 distance >= that, i.e. a true distance >= bound * (1 - 1e-5), so it cannot
// belong to the k nearest -- and (ii) it is no larger than the distance to the region's border, so nothing outside the region can
// either.  The rest is listed for the per-lane search.
template <int KMAX, bool NORMALS = false>
__global__ void __launch_bounds__(128) covariance_settle_kernel(const float4* __restrict__ sorted, RowScanOut in, const float* __restrict__ points, int k,
                                                                float* __restrict__ covs, int* __restrict__ todo_list, int* __restrict__ todo_count,
                                                                float* __restrict__ normals = nullptr) {
  static_assert(KMAX + 2 <= kTileKeep, "two entries of slack");
  const int pos = blockIdx.x * 128 + threadIdx.x;
  const bool active = pos < in.nq;
  bool leftover = false;
  if (active) {
    const float bound = in.bound[pos];
    leftover = true;
    if (bound >= 0.0f) {
      const float4 self = sorted[pos];
      const double q[3] = {(double)self.x, (double)self.y, (double)self.z};
      TopK<KMAX> exact;
      exact.init(k, 1.7976931348623157e308);
      int idx[kTileKeep];
#pragma unroll
      for (int j = 0; j < kTileKeep; j++) idx[j] = in.kept[(size_t)j * in.nq + pos];
#pragma unroll
      for (int j = 0; j < kTileKeep; j++) {
        if (idx[j] >= 0) {
          const size_t nb = (size_t)idx[j];
          const double ddx = (double)points[3 * nb] - q[0], ddy = (double)points[3 * nb + 1] - q[1], ddz = (double)points[3 * nb + 2] - q[2];
          exact.push(idx[j], ddx * ddx + ddy * ddy + ddz * ddz);
        }
      }
      const double safe = (double)in.safe[pos];
      const bool separated = exact.worst() <= (double)bound * (1.0 - 1.0e-5);
      if (exact.found >= k && separated && exact.worst() <= safe * safe) {
        const size_t i = (size_t)__float_as_int(self.w);
        covariance_from_neighbours<KMAX, false, NORMALS>(exact, points, k, (!NORMALS || covs) ? covs + 9 * i : nullptr, NORMALS ? normals + 3 * i : nullptr, q[0], q[1], q[2]);
        leftover = false;
      }
    }
  }
  todo_append(leftover, pos, todo_list, todo_count);
}

}  // namespace gp
