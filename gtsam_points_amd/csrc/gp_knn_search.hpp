// gp_knn_search.hpp -- the device side of the exact k-nearest-neighbour search: the TopK list and the walkers over the structures of gp_knn_grid.hpp
// (knn_query / knn_query_multi on the hashed grid; knn_query_bins, knn_query_octant and knn_query_coarse on the binned grid; knn_query_any picks).
// Device code only, no kernels: gp_knn.hip (search, mean neighbour distance, correspondences) and gp_covariance.hip (covariances, normals) call it.
//
// Replaces (reference, CPU only -- there is no GPU counterpart upstream):
//   ann/small_kdtree.hpp:124-186,437-474 + ann/knn_result.hpp:89-109   exact k-NN (kd-tree)      -> uniform-grid shell search
//
// Exactness: a query visits the cells of growing cubes around its own cell and stops after radius r once it holds k
// neighbours whose k-th squared distance is <= d_safe(r)^2, where d_safe(r) = r*h + (distance from the query to the
// nearest face of its own cell) is a lower bound on the distance to every unvisited point.  Distances are computed in
// f64 on the f32 inputs (as the reference does on PointCloudCPU's doubles), so the neighbour SET equals the kd-tree's
// except for exact ties at the k-th distance (where the reference's own result depends on traversal order).
#pragma once

#include "gp_knn_grid.hpp"

namespace gp {

// ---- exact k-NN -------------------------------------------------------------------------------------------------
template <int KMAX, bool FULL = false>  // FULL: the list always holds exactly KMAX neighbours (k == KMAX): straight-line insertion only
struct TopK {
  // d / idx are only ever indexed with compile-time constants (unrolled loops + predicates): a run-time index such as d[k - 1]
  // would send both arrays to scratch memory (160 B per lane for KMAX = 10) and turn every comparison into a memory access
  double d[KMAX];
  int idx[KMAX];
  double bound;  // = d[k - 1]: the current k-th distance (or the caller's max_sq_dist while fewer than k are held)
  int k, found;
  __device__ void init(int k_, double max_sq_dist) {
    k = k_;
    found = 0;
    bound = max_sq_dist;
#pragma unroll
    for (int j = 0; j < KMAX; j++) {
      d[j] = max_sq_dist;
      idx[j] = -1;
    }
  }
  __device__ double worst() const { return bound; }
  // neighbours held.  FULL lists do not count their insertions (two instructions in the hottest block of the search): an entry is held iff its index is valid
  __device__ int count() const {
    if constexpr (FULL) {
      int c = 0;
#pragma unroll
      for (int j = 0; j < KMAX; j++) c += idx[j] >= 0 ? 1 : 0;
      return c;
    } else {
      return found;
    }
  }
  // KnnResult::push (ann/knn_result.hpp:89-109): strict '<', earlier-visited ties win
  __device__ void push(int index, double dist) {
    if (!(dist < bound)) return;
    if constexpr (FULL) {
      // full list (the common case: covariance estimation asks for exactly KMAX): straight-line code.  c[j] = dist < d[j] is monotone in j (the list is
      // sorted), the new entry j is d[j-1] where c[j-1], the candidate where c[j] alone, d[j] otherwise -- for the distances that is
      // max(d[j-1], min(dist, d[j])), for the indices two selects on the same masks: 10 compares + 20 min/max + 20 selects, no exec-mask regions
      // (the position-by-position form below compiles to ten of them plus a scalar branch tree for the bound: ~70 vector and ~80 scalar / branch
      // instructions per insertion, executed by the whole wave whenever one lane inserts)
      bool c[KMAX];
#pragma unroll
      for (int j = 0; j < KMAX; j++) c[j] = dist < d[j];
      // (v_min_f64 / v_max_f64 through asm: fmin / fmax make hipcc quiet every operand first -- `v_max_f64 x, x, x`, eleven more f64 instructions per
      // insertion -- and no operand here is a NaN: squared distances of finite points and the finite sentinel of init())
      auto min64 = [](double a, double b) {
        double r;
        asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
        return r;
      };
      auto max64 = [](double a, double b) {
        double r;
        asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
        return r;
      };
#pragma unroll
      for (int j = KMAX - 1; j >= 1; j--) {
        idx[j] = c[j - 1] ? idx[j - 1] : (c[j] ? index : idx[j]);
        d[j] = max64(d[j - 1], min64(dist, d[j]));
      }
      idx[0] = c[0] ? index : idx[0];
      d[0] = min64(dist, d[0]);
      bound = d[KMAX - 1];
      return;  // (`found` is not kept up in this form: count() reads it off the list)
    }
    bool placed = false;
#pragma unroll
    for (int j = KMAX - 1; j >= 0; j--) {
      if (j < k && !placed) {
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
#pragma unroll
    for (int j = 0; j < KMAX; j++)
      if (j == k - 1) bound = d[j];
    found = found + 1 < k ? found + 1 : k;
  }
};

// f32 filter bound for "exact squared distance < worst": the f32 differences are off by <= m per axis, so the f32 squared distance is at most
// worst (1 + 1e-6) + 4 sqrt(worst) m + 4 m^2, and 4 sqrt(w) m <= w / 1024 + 4096 m^2 (AM-GM) spares the square root -- it sat behind every insertion
// with its IEEE refinement, ~20 instructions; the filter admits candidates within 0.1 % of the bound instead, the f64 comparison decides as before
__device__ __forceinline__ float loosened_bound(double worst, float m2x4100) { return (float)worst * 1.000978f + m2x4100; }

template <int KMAX, bool FULL>
__device__ __forceinline__ void knn_query(const GridView& g, double qx, double qy, double qz, TopK<KMAX, FULL>& top);

__device__ __forceinline__ int count27(const GridView& g, double qx, double qy, double qz) {
  const int cx = hashed_cell(qx * g.inv_h), cy = hashed_cell(qy * g.inv_h), cz = hashed_cell(qz * g.inv_h);
  int c = 0;
  for (int dz = -1; dz <= 1; dz++)
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        const int s = grid_find(g, pack_cell(cx + dx, cy + dy, cz + dz));
        if (s >= 0) c += g.start[s + 1] - g.start[s];
      }
  return c;
}

template <int KMAX, bool FULL>
__device__ __forceinline__ void knn_query_multi(const MultiGridView& mg, double qx, double qy, double qz, int want, TopK<KMAX, FULL>& top) {
  int level = mg.num_levels - 1;
  for (int l = 0; l + 1 < mg.num_levels; l++) {
    if (count27(mg.lv[l], qx, qy, qz) >= want) {
      level = l;
      break;
    }
  }
  knn_query<KMAX, FULL>(mg.lv[level], qx, qy, qz, top);
}

template <int KMAX, bool FULL>
__device__ __forceinline__ void knn_query(const GridView& g, double qx, double qy, double qz, TopK<KMAX, FULL>& top) {
  if (!(fabs(qx) < 1.0e300 && fabs(qy) < 1.0e300 && fabs(qz) < 1.0e300)) return;  // non-finite query: no neighbours
  const int cx = hashed_cell(qx * g.inv_h), cy = hashed_cell(qy * g.inv_h), cz = hashed_cell(qz * g.inv_h);
  // distance from the query to the nearest face of its own cell
  const double fx = qx * g.inv_h - (double)cx, fy = qy * g.inv_h - (double)cy, fz = qz * g.inv_h - (double)cz;
  const double face = fmin(fmin(fmin(fx, 1.0 - fx), fmin(fy, 1.0 - fy)), fmin(fz, 1.0 - fz)) * g.h;
  // cube radius after which every occupied cell has been visited from this query
  const int rmax = max(max(max(abs(cx - g.lo[0]), abs(cx - g.hi[0])), max(abs(cy - g.lo[1]), abs(cy - g.hi[1]))), max(abs(cz - g.lo[2]), abs(cz - g.hi[2])));
  for (int r = 0; r <= rmax; r++) {
    for (int dz = -r; dz <= r; dz++)
      for (int dy = -r; dy <= r; dy++) {
        const bool shell_yz = (dz == -r || dz == r || dy == -r || dy == r);
        const int step = (shell_yz || r == 0) ? 1 : 2 * r;  // interior rows: only dx = -r and dx = +r belong to the shell
        for (int dx = -r; dx <= r; dx += step) {
          const int s = grid_find(g, pack_cell(cx + dx, cy + dy, cz + dz));
          if (s < 0) continue;
          const int b = g.start[s], e = g.start[s + 1];
          for (int p = b; p < e; p++) {
            const float4 v = g.sorted[p];
            const double ddx = (double)v.x - qx, ddy = (double)v.y - qy, ddz = (double)v.z - qz;
            top.push(__float_as_int(v.w), ddx * ddx + ddy * ddy + ddz * ddz);
          }
        }
      }
    const double safe = (double)r * g.h + face;
    if (top.worst() <= safe * safe) return;  // every unvisited point is farther than the current k-th (or than max_sq_dist)
    if (top.count() >= g.n) return;            // the whole cloud has been seen (clouds smaller than k)
  }
}

// ---- search over the binned structure (gp_binning.hpp): occupancy-block grid over the cells + cell-sorted points -------------------
// A query walks the cube shells around its cell like knn_query above, but reads ONE 16-B block entry per 4 x 4 x 4 cells instead of
// probing a hash table per cell, visits only occupied cells (bit scan), and filters candidates with an f32 distance before the f64
// distance that decides (the reference compares doubles): the shell loop of a typical query touches <= 8 block entries.
// 4-bit mask of the cells x = 4 * b + {0, 1, 2, 3} inside [c - r, c + r]
__device__ __forceinline__ unsigned axis_mask(int b, int c, int r) {
  int lo = c - r - 4 * b, hi = c + r - 4 * b;
  lo = lo < 0 ? 0 : lo;
  hi = hi > 3 ? 3 : hi;
  return lo > hi ? 0u : (((2u << hi) - 1u) & ~((1u << lo) - 1u));
}
// 64-bit cell mask of a block from its per-axis 4-bit masks (bit = z * 16 + y * 4 + x)
__device__ __forceinline__ unsigned long long cube_mask(unsigned mx, unsigned my, unsigned mz) {
  const unsigned long long X = (unsigned long long)mx * 0x1111111111111111ull;
  const unsigned y4 = (my & 1u) | ((my & 2u) << 3) | ((my & 4u) << 6) | ((my & 8u) << 9);  // bit y -> bit 4 y
  const unsigned long long Y = (unsigned long long)(y4 * 0xFu) * 0x0001000100010001ull;
  const unsigned long long z1 = (unsigned long long)mz;
  const unsigned long long Z = ((z1 | (z1 << 15) | (z1 << 30) | (z1 << 45)) & 0x0001000100010001ull) * 0xFFFFull;
  return X & Y & Z;
}

// max_shells: how many shells beyond the first one that reaches the box this call may walk before it gives up (returns false: the
// caller retries on a coarser level); returns true when the search is complete (bound met, or every point seen)
constexpr int kDeferShell = 2;      // (covariance search with the cooperative pass) a query with fewer than k points within this many cells of its cell is deferred
constexpr int kRangeCap = 16;       // candidate ranges a lane collects before it scans them (flat scan of knn_query_bins)
constexpr int kFlatWidth = 4;       // candidates whose loads a lane has in flight per trip of the flat scan (8: 16 registers spilled, 0.748 vs 0.754 ms per call: no gain)
constexpr int kRangeStride = 128;   // int2 entries between two slots of one lane's list = threads of the workgroups that use it

// (round 5: a query the fine shells cannot settle -- knn_query_any's `sparse` -- is not continued on the coarser levels lane by lane but handed to covariance_far_kernel)
template <int KMAX, bool FULL, bool FLAT = false>
__device__ __forceinline__ bool knn_query_bins(const BinGridView& g, double qx, double qy, double qz, TopK<KMAX, FULL>& top, int max_shells, int2* rl = nullptr,
                                               bool* sparse = nullptr) {
  const double ux = qx * g.inv_h, uy = qy * g.inv_h, uz = qz * g.inv_h;
  if (!cell_in_range(ux, uy, uz)) return true;  // non-finite query: no neighbours
  const int c[3] = {fast_floor(ux), fast_floor(uy), fast_floor(uz)};
  const double fx = ux - (double)c[0], fy = uy - (double)c[1], fz = uz - (double)c[2];
  const double face = fmin(fmin(fmin(fx, 1.0 - fx), fmin(fy, 1.0 - fy)), fmin(fz, 1.0 - fz)) * g.h;
  int lo[3], hi[3], r0 = 0, rmax = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = g.geom.lo[a] * 4;
    hi[a] = (g.geom.lo[a] + g.geom.dim[a]) * 4 - 1;
    r0 = max(r0, max(lo[a] - c[a], c[a] - hi[a]));              // first shell that reaches the box
    rmax = max(rmax, max(abs(c[a] - lo[a]), abs(c[a] - hi[a])));  // shell that covers it
  }
  const float qxf = (float)qx, qyf = (float)qy, qzf = (float)qz;
  const float fxf = (float)fx, fyf = (float)fy, fzf = (float)fz, h2f = (float)(g.h * g.h);  // (cell-box pruning below)
  // |f32 difference - exact difference| <= margin per axis (rounding of q to float + the subtraction), generously
  const float margin = (fabsf(qxf) + fabsf(qyf) + fabsf(qzf) + 1.0f) * 2.4e-7f;
  const float m2x4100 = 4100.0f * margin * margin;
  auto loosened = [&](double worst) { return loosened_bound(worst, m2x4100); };  // (+inf while fewer than k neighbours are held and no distance bound was given)
  float accept = loosened(top.worst());
  unsigned n_f32 = 0, n_f64 = 0, n_blk = 0, n_cell = 0;  // work counters: only read when g.counters is set (measurement runs)
  // candidates of one cell: the loads of four consecutive points are issued together (a lane's loads miss L1 more often than not, and
  // one round trip per point was the whole cost of this search), the tests follow in point order
  auto test_point = [&](const float4 v) {
    const float dxf = v.x - qxf, dyf = v.y - qyf, dzf = v.z - qzf;
    if (dxf * dxf + dyf * dyf + dzf * dzf <= accept) {
      n_f64++;
      const double ddx = (double)v.x - qx, ddy = (double)v.y - qy, ddz = (double)v.z - qz;
      top.push(__float_as_int(v.w), ddx * ddx + ddy * ddy + ddz * ddz);
      accept = loosened(top.worst());
    }
  };
  auto scan_range = [&](int pb, int pe) {
    int p = pb;
    for (; p + 4 <= pe; p += 4) {
      const float4 v0 = g.sorted[p], v1 = g.sorted[p + 1], v2 = g.sorted[p + 2], v3 = g.sorted[p + 3];
      test_point(v0);
      test_point(v1);
      test_point(v2);
      test_point(v3);
    }
    if (p < pe) {
      const int last = pe - 1;
      const float4 v0 = g.sorted[p], v1 = g.sorted[min(p + 1, last)], v2 = g.sorted[min(p + 2, last)];
      test_point(v0);
      if (p + 1 < pe) test_point(v1);
      if (p + 2 < pe) test_point(v2);
    }
  };
  // FLAT scan (rl != nullptr: a per-lane list of candidate ranges in LDS, kRangeCap entries, lane stride kRangeStride).  Scanning a cell the moment the walk
  // finds it keeps the lanes of a wave out of step -- they find their cells at different points of the nested block / cell loops, and the wave runs the point
  // loop once per (lane group, cell): ~590 executions of the candidate test per wave for ~185 candidates per lane.  With the list, a shell's cells are only
  // COLLECTED by the walk; then every lane streams through its ranges in one loop, four candidates per trip, all lanes busy until their own list ends.  A
  // lane's candidates keep their order, so the result is the same list, bit for bit.
  int rl_count = 0;
  auto flush_ranges = [&]() {
    int ri = 0, p = 0, pe = 0;
    auto next_range = [&]() {
      p = 0;
      pe = 0;
      while (ri < rl_count) {
        const int2 rg = rl[ri * kRangeStride];
        ri++;
        // round 4: a cell collected while the list was not full yet (or the bound still loose) is looked at again when its turn comes: by then a dense cell in front of
        // it has usually brought the k-th distance down to centimetres, and a cell whose box is farther than that holds nothing of interest -- the queries that needed
        // shell 1 because their own cell held fewer than k points used to scan all 26 neighbours in full (up to 465 candidates on a lane, the launch's longest waves)
        if (__int_as_float(rg.y & (int)0xffff0000) > accept) continue;
        p = rg.x;
        pe = rg.x + (rg.y & 0xffff);
        break;
      }
    };
    next_range();
    while (p < pe) {
      int a[kFlatWidth];
      bool k[kFlatWidth];
#pragma unroll
      for (int q = 0; q < kFlatWidth; q++) {
        a[q] = 0;
        k[q] = p < pe;
        if (k[q]) {
          a[q] = p;
          p++;
          if (p == pe) next_range();
        }
      }
      float4 v[kFlatWidth];
#pragma unroll
      for (int q = 0; q < kFlatWidth; q++) v[q] = g.sorted[a[q]];
#pragma unroll
      for (int q = 0; q < kFlatWidth; q++)
        if (k[q]) test_point(v[q]);
    }
    rl_count = 0;
  };
  // box2: squared distance of the cell's box from the query (0 for the own cell), already scaled down by the slack of the collection-time test; kept with the range as
  // the upper 16 bits of a float -- truncated, i.e. rounded DOWN: the re-test at scan time can only keep more than the exact value would -- beside a 16-bit count
  auto visit_range = [&](int pb, int pe, float box2) {
    if constexpr (!FLAT) {
      scan_range(pb, pe);
    } else {
      while (pe > pb) {
        const int cnt = min(pe - pb, 0xffff);
        rl[rl_count * kRangeStride] = make_int2(pb, cnt | (__float_as_int(box2) & (int)0xffff0000));
        rl_count++;
        pb += cnt;
        if (__builtin_amdgcn_ballot_w64(rl_count >= kRangeCap) != 0ull) flush_ranges();  // (some lane's list is full: the lanes that are here scan what they hold)
      }
    }
  };
  const int rlast = (max_shells < rmax - r0) ? r0 + max_shells : rmax;
  for (int r = r0; r <= rlast; r++) {
    int b0[3], b1[3];
    bool any = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const int x0 = max(c[a] - r, lo[a]), x1 = min(c[a] + r, hi[a]);
      any = any && x0 <= x1;
      b0[a] = x0 >> 2;
      b1[a] = x1 >> 2;
    }
    // Round 5: NEAR CELLS FIRST for the queries that reach shell 1 with a list that is not full (own cell < k points).  Next to a dense surface those were the launch's
    // longest waves after the far field: with no bound yet they collected all 26 neighbours in walk order and scanned 250-470 candidates per lane, the far corner cells in
    // full before the near face cell had filled the list (profiles/r04_c5_wavelog.txt: 500-545 us per wave against a mean of 107).  They walk the shell TWICE: pass 0
    // takes the cells whose box lies within half a cell edge of the query (the octant it leans to: <= 7 cells), the list is scanned, and pass 1 meets the rest with the
    // k-th distance those brought -- most of it fails the box test below before its range is even looked up.  Queries whose list is full walk once, as before (walking
    // everybody twice: the same lists, 5 % more wave time; one walk with the near ranges sorted to the front of the 16-entry list: no gain, the near cell is often not
    // among the first 16 -- profiles/r05_c5_near_first.txt).  Same candidates, same k smallest; only exact ties in distance could tell the visiting orders apart.
    const int passes = (FLAT && r == 1 && top.count() < top.k) ? 2 : 1;
    const float near2 = 0.25f * h2f;
    if (any)
     for (int pass = 0; pass < passes; pass++) {
      // only blocks that touch the shell are visited: a z-slab of blocks that lies inside the previous cube along z contributes
      // its y-border rows, and such a row its two x-border blocks (surface, not volume, per shell)
      for (int bz = b0[2]; bz <= b1[2]; bz++) {
        const unsigned mz = axis_mask(bz, c[2], r), mz1 = r > 0 ? axis_mask(bz, c[2], r - 1) : 0u;
        const bool zin = mz1 == 0xFu;
        for (int by = b0[1]; by <= b1[1]; by++) {
          const unsigned my = axis_mask(by, c[1], r), my1 = r > 0 ? axis_mask(by, c[1], r - 1) : 0u;
          const bool yin = zin && my1 == 0xFu;
          const int xstep = (yin && b1[0] > b0[0]) ? b1[0] - b0[0] : 1;  // interior row: first and last block only
          for (int bx = b0[0]; bx <= b1[0]; bx += xstep) {
            const unsigned mx = axis_mask(bx, c[0], r), mx1 = r > 0 ? axis_mask(bx, c[0], r - 1) : 0u;
            if (mx1 == 0xFu && my1 == 0xFu && mz1 == 0xFu) continue;  // the whole block lies inside the previous cube
            const size_t bi = ((size_t)(bz - g.geom.lo[2]) * (size_t)g.geom.dim[1] + (size_t)(by - g.geom.lo[1])) * (size_t)g.geom.dim[0] + (size_t)(bx - g.geom.lo[0]);
            const int4 raw = *reinterpret_cast<const int4*>(g.blocks + bi);
            n_blk++;
            const unsigned long long bits = ((unsigned long long)(unsigned)raw.y << 32) | (unsigned long long)(unsigned)raw.x;
            if (bits == 0ull) continue;  // an empty block (most of what a far-field query walks): nothing to mask
            unsigned long long m = bits & cube_mask(mx, my, mz) & ~cube_mask(mx1, my1, mz1);  // occupied cells of this shell
            while (m) {
              const int bit = __ffsll((long long)m) - 1;
              m &= m - 1ull;
              float box2 = 0.0f;
              if (r > 0) {
                // a cell whose box is farther from the query than the current k-th neighbour holds nothing of interest (the corners of a shell's cube
                // usually are): box distance in cell units, f32 with slack -- the test only ever SKIPS, and only cells every point of which fails the
                // list's own strict comparison
                // (relative to the query's own cell: small integers and the query's position inside its cell, exact to 1e-7 whatever the coordinates)
                const float rx = (float)(4 * bx + (bit & 3) - c[0]) - fxf, ry = (float)(4 * by + ((bit >> 2) & 3) - c[1]) - fyf, rz = (float)(4 * bz + (bit >> 4) - c[2]) - fzf;
                const float ex = fmaxf(fmaxf(rx, -rx - 1.0f), 0.0f), ey = fmaxf(fmaxf(ry, -ry - 1.0f), 0.0f), ez = fmaxf(fmaxf(rz, -rz - 1.0f), 0.0f);
                box2 = (ex * ex + ey * ey + ez * ez) * h2f * 0.9999f;
                if (passes == 2 && (box2 <= near2) != (pass == 0)) continue;  // (not this pass's)
                if (box2 > accept) continue;
              }
              const int ord = raw.z + __popcll(bits & ((1ull << bit) - 1ull));
              const int pb = g.cell_start[ord], pe = g.cell_start[ord + 1];
              n_cell++;
              n_f32 += (unsigned)(pe - pb);
              visit_range(pb, pe, box2);
            }
          }
        }
      }
      if constexpr (FLAT) {
        if (pass + 1 < passes) flush_ranges();
      }
     }
    if constexpr (FLAT) flush_ranges();
    const double safe = (double)r * g.h + face;
    const bool done = top.worst() <= safe * safe   // every unvisited point is farther than the current k-th (or than max_sq_dist)
                      || top.count() >= g.n;         // the whole cloud has been seen (clouds smaller than k)
    // (round 5: fewer than k points within kDeferShell cells of the query's cell -- the cells are the wrong tool here, and one lane walking on keeps its wave's other
    // 63 waiting: the caller hands the query to covariance_far_kernel)
    if (sparse && !done && r >= kDeferShell && r < rlast && top.count() < top.k) {
      *sparse = true;
      return false;
    }

    if (done || r == rlast) {
      if (g.counters) {
        atomicAdd(g.counters + 0, 1ull);
        atomicAdd(g.counters + 1, (unsigned long long)n_f32);
        atomicAdd(g.counters + 2, (unsigned long long)n_f64);
        atomicAdd(g.counters + 3, (unsigned long long)n_blk);
        atomicAdd(g.counters + 4, (unsigned long long)n_cell);
      }
      return done || rlast >= rmax;
    }
  }
  return rlast >= rmax;  // (r0 > rlast: nothing to walk)
}

// First stage of a 1-NN search (GICP correspondences): the 2 x 2 x 2 cells nearest to the query -- its own cell and, per axis, the
// neighbour on the side the query leans to.  Every point within min over the axes of max(f, 1 - f) >= 1/2 cells (f = the query's
// position inside its cell) is in there, and a matched point's neighbour is a few centimetres away, so this settles almost every query with 8 cells instead of the
// 27 of shells 0 + 1.  The 8 block entries are requested together, then the 8 cell ranges, then the points four at a time: three
// dependent round trips in front of the point scan instead of one per block, cell and point.  Returns true when the bound is met;
// otherwise the caller walks the shells with the list as it stands (a point pushed twice cannot displace itself in a 1-NN list).
template <int KMAX, bool FULL>
__device__ __forceinline__ bool knn_query_octant(const BinGridView& g, double qx, double qy, double qz, TopK<KMAX, FULL>& top) {
  static_assert(KMAX == 1, "duplicates are harmless only in a 1-NN list");
  const double ux = qx * g.inv_h, uy = qy * g.inv_h, uz = qz * g.inv_h;
  if (!cell_in_range(ux, uy, uz)) return true;  // non-finite query: no neighbours
  const int c[3] = {fast_floor(ux), fast_floor(uy), fast_floor(uz)};
  const double f[3] = {ux - (double)c[0], uy - (double)c[1], uz - (double)c[2]};
  int o[3];
  double reach = 1.0e300;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    o[a] = f[a] < 0.5 ? -1 : 1;
    reach = fmin(reach, fmax(f[a], 1.0 - f[a]));  // distance (cells) to the nearer end of the two-cell span along this axis
  }
  const float qxf = (float)qx, qyf = (float)qy, qzf = (float)qz;
  const float margin = (fabsf(qxf) + fabsf(qyf) + fabsf(qzf) + 1.0f) * 2.4e-7f;  // as in knn_query_bins
  const float m2x4100 = 4100.0f * margin * margin;
  auto loosened = [&](double worst) { return loosened_bound(worst, m2x4100); };
  float accept = loosened(top.worst());
  unsigned n_f32 = 0, n_f64 = 0, n_cell = 0;
  int4 e[8];
  int bit[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int cx = c[0] + ((i & 1) ? o[0] : 0), cy = c[1] + ((i & 2) ? o[1] : 0), cz = c[2] + ((i & 4) ? o[2] : 0);
    const int bx = (cx >> 2) - g.geom.lo[0], by = (cy >> 2) - g.geom.lo[1], bz = (cz >> 2) - g.geom.lo[2];
    bit[i] = (cx & 3) | ((cy & 3) << 2) | ((cz & 3) << 4);
    const bool in = bx >= 0 && bx < g.geom.dim[0] && by >= 0 && by < g.geom.dim[1] && bz >= 0 && bz < g.geom.dim[2];
    e[i] = in ? *reinterpret_cast<const int4*>(g.blocks + ((size_t)bz * (size_t)g.geom.dim[1] + (size_t)by) * (size_t)g.geom.dim[0] + (size_t)bx) : make_int4(0, 0, 0, 0);
  }
  int pb[8], pe[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const unsigned long long bits = ((unsigned long long)(unsigned)e[i].y << 32) | (unsigned long long)(unsigned)e[i].x;
    const bool occ = (bits >> bit[i]) & 1ull;
    const int ord = e[i].z + __popcll(bits & ((1ull << bit[i]) - 1ull));
    pb[i] = occ ? g.cell_start[ord] : 0;
    pe[i] = occ ? g.cell_start[ord + 1] : 0;
  }
  auto test_point = [&](const float4 v) {
    const float dxf = v.x - qxf, dyf = v.y - qyf, dzf = v.z - qzf;
    if (dxf * dxf + dyf * dyf + dzf * dzf <= accept) {
      n_f64++;
      const double ddx = (double)v.x - qx, ddy = (double)v.y - qy, ddz = (double)v.z - qz;
      top.push(__float_as_int(v.w), ddx * ddx + ddy * ddy + ddz * ddz);
      accept = loosened(top.worst());
    }
  };
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if (pe[i] > pb[i]) {
      n_cell++;
      n_f32 += (unsigned)(pe[i] - pb[i]);
      const int last = pe[i] - 1;
      for (int p = pb[i]; p < pe[i]; p += 4) {
        const float4 v0 = g.sorted[p], v1 = g.sorted[min(p + 1, last)], v2 = g.sorted[min(p + 2, last)], v3 = g.sorted[min(p + 3, last)];
        test_point(v0);  // (the clamped repeats of the last point are harmless in a 1-NN list)
        test_point(v1);
        test_point(v2);
        test_point(v3);
      }
    }
  }
  if (g.counters) {
    atomicAdd(g.counters + 5, 1ull);
    atomicAdd(g.counters + 1, (unsigned long long)n_f32);
    atomicAdd(g.counters + 2, (unsigned long long)n_f64);
    atomicAdd(g.counters + 3, 8ull);
    atomicAdd(g.counters + 4, (unsigned long long)n_cell);
  }
  const double safe = reach * g.h;
  return top.worst() <= safe * safe;
}

// The same exact search one and two levels up WITHOUT further sorted copies: the 4 x 4 x 4-cell blocks of the grid are the cells of a
// grid with four times the cell size, and because the points are sorted by (block, cell) a block's points are ONE contiguous range
// of the sorted array -- [cell_start[base], cell_start[base + popcount(bits)]).  Queries whose neighbourhood is too sparse for the
// fine shells (far field of a LiDAR scan) walk cube shells of blocks here, surface only.  SUPER: the cells are 4 x 4 x 4 BLOCKS
// (16 x the cell size) and an entry is the 64-bit occupancy mask of its blocks (BinGridView::super) -- isolated points walk hundreds
// of shells' worth of empty space in a few dozen 8-byte loads this way.  Entries of an x-row are contiguous in memory and are
// requested four at a time: one round trip per (mostly empty) entry was what these walks cost.
// Returns true when the search is complete (bound met, every point seen, or the box exhausted), false after max_shells + 1 shells.
template <int KMAX, bool SUPER, bool FULL>
__device__ __forceinline__ bool knn_query_coarse(const BinGridView& g, double qx, double qy, double qz, TopK<KMAX, FULL>& top, int max_shells) {
  const double unit = (SUPER ? 16.0 : 4.0) * g.h, inv_unit = (SUPER ? 0.0625 : 0.25) * g.inv_h;
  // SUPER coordinates are relative to the grid's first block (the grid origin is not a multiple of four blocks)
  const double ux = qx * inv_unit - (SUPER ? 0.25 * (double)g.geom.lo[0] : 0.0), uy = qy * inv_unit - (SUPER ? 0.25 * (double)g.geom.lo[1] : 0.0),
               uz = qz * inv_unit - (SUPER ? 0.25 * (double)g.geom.lo[2] : 0.0);
  if (!cell_in_range(ux, uy, uz)) return true;
  const int c[3] = {fast_floor(ux), fast_floor(uy), fast_floor(uz)};
  const double fx = ux - (double)c[0], fy = uy - (double)c[1], fz = uz - (double)c[2];
  const double face = fmin(fmin(fmin(fx, 1.0 - fx), fmin(fy, 1.0 - fy)), fmin(fz, 1.0 - fz)) * unit;
  int lo[3], hi[3], r0 = 0, rmax = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = SUPER ? 0 : g.geom.lo[a];
    hi[a] = SUPER ? g.sdim[a] - 1 : g.geom.lo[a] + g.geom.dim[a] - 1;
    r0 = max(r0, max(lo[a] - c[a], c[a] - hi[a]));
    rmax = max(rmax, max(abs(c[a] - lo[a]), abs(c[a] - hi[a])));
  }
  const int dimx = SUPER ? g.sdim[0] : g.geom.dim[0], dimy = SUPER ? g.sdim[1] : g.geom.dim[1];
  const float qxf = (float)qx, qyf = (float)qy, qzf = (float)qz;
  const float margin = (fabsf(qxf) + fabsf(qyf) + fabsf(qzf) + 1.0f) * 2.4e-7f;  // as in knn_query_bins
  const float m2x4100 = 4100.0f * margin * margin;
  auto loosened = [&](double worst) { return loosened_bound(worst, m2x4100); };
  float accept = loosened(top.worst());
  unsigned n_f32 = 0, n_f64 = 0, n_blk = 0;
  auto test_point = [&](const float4 v) {
    const float dxf = v.x - qxf, dyf = v.y - qyf, dzf = v.z - qzf;
    if (dxf * dxf + dyf * dyf + dzf * dzf <= accept) {
      n_f64++;
      const double ddx = (double)v.x - qx, ddy = (double)v.y - qy, ddz = (double)v.z - qz;
      top.push(__float_as_int(v.w), ddx * ddx + ddy * ddy + ddz * ddz);
      accept = loosened(top.worst());
    }
  };
  auto scan_block = [&](const int4 raw) {
    const unsigned long long bits = ((unsigned long long)(unsigned)raw.y << 32) | (unsigned long long)(unsigned)raw.x;
    if (bits == 0ull) return;
    const int pb = g.cell_start[raw.z], pe = g.cell_start[raw.z + __popcll(bits)];
    n_f32 += (unsigned)(pe - pb);
    int p = pb;
    for (; p + 4 <= pe; p += 4) {  // four loads in flight (a block holds a few hundred points at most)
      const float4 v0 = g.sorted[p], v1 = g.sorted[p + 1], v2 = g.sorted[p + 2], v3 = g.sorted[p + 3];
      test_point(v0);
      test_point(v1);
      test_point(v2);
      test_point(v3);
    }
    for (; p < pe; p++) test_point(g.sorted[p]);
  };
  auto scan_super = [&](unsigned long long m, int sx, int sy, int sz) {  // occupied blocks of superblock (sx, sy, sz)
    while (m) {
      const int bit = __ffsll((long long)m) - 1;
      m &= m - 1ull;
      const int bx = 4 * sx + (bit & 3), by = 4 * sy + ((bit >> 2) & 3), bz = 4 * sz + (bit >> 4);
      // a block farther away than the current k-th neighbour holds nothing of interest
      const double e = 4.0 * g.h;
      const double x0 = (double)(g.geom.lo[0] + bx) * e, y0 = (double)(g.geom.lo[1] + by) * e, z0 = (double)(g.geom.lo[2] + bz) * e;
      const double ddx = fmax(fmax(x0 - qx, qx - (x0 + e)), 0.0), ddy = fmax(fmax(y0 - qy, qy - (y0 + e)), 0.0), ddz = fmax(fmax(z0 - qz, qz - (z0 + e)), 0.0);
      if (ddx * ddx + ddy * ddy + ddz * ddz > top.worst()) continue;
      n_blk++;
      scan_block(*reinterpret_cast<const int4*>(g.blocks + ((size_t)bz * (size_t)g.geom.dim[1] + (size_t)by) * (size_t)g.geom.dim[0] + (size_t)bx));
    }
  };
  // entries xa .. xb (step `step`) of one x-row
  auto visit_row = [&](int xa, int xb, int step, int y, int z) {
    const size_t row0 = ((size_t)(z - lo[2]) * (size_t)dimy + (size_t)(y - lo[1])) * (size_t)dimx;
    for (int x = xa; x <= xb; x += 4 * step) {
      if constexpr (SUPER) {
        unsigned long long e[4];
#pragma unroll
        for (int i = 0; i < 4; i++) e[i] = g.super[row0 + (size_t)(min(x + i * step, xb) - lo[0])];
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (x + i * step <= xb) scan_super(e[i], x + i * step, y, z);
      } else {
        int4 e[4];
#pragma unroll
        for (int i = 0; i < 4; i++) e[i] = *reinterpret_cast<const int4*>(g.blocks + row0 + (size_t)(min(x + i * step, xb) - lo[0]));
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (x + i * step <= xb) {
            n_blk++;
            scan_block(e[i]);
          }
      }
    }
  };
  bool done = false;
  const int rlast = (max_shells < rmax - r0) ? r0 + max_shells : rmax;
  for (int r = r0; r <= rlast && !done; r++) {
    const int z0 = max(c[2] - r, lo[2]), z1 = min(c[2] + r, hi[2]);
    const int y0 = max(c[1] - r, lo[1]), y1 = min(c[1] + r, hi[1]);
    const int x0 = max(c[0] - r, lo[0]), x1 = min(c[0] + r, hi[0]);
    if (z0 <= z1 && y0 <= y1 && x0 <= x1) {
      for (int z = z0; z <= z1; z++) {
        const bool zface = z == c[2] - r || z == c[2] + r;
        for (int y = y0; y <= y1; y++) {
          if (zface || y == c[1] - r || y == c[1] + r || r == 0) {
            visit_row(x0, x1, 1, y, z);
          } else {  // interior row of the cube: only its two end entries belong to the shell
            const int xa = c[0] - r >= lo[0] ? c[0] - r : c[0] + r, xb = c[0] + r <= hi[0] ? c[0] + r : c[0] - r;
            if (xa >= lo[0] && xa <= hi[0] && xb >= xa) visit_row(xa, xb, xb > xa ? xb - xa : 1, y, z);
          }
        }
      }
    }
    const double safe = (double)r * unit + face;
    done = top.worst() <= safe * safe || top.count() >= g.n;
  }
  if (g.counters) {
    atomicAdd(g.counters + 0, 1ull);
    atomicAdd(g.counters + 1, (unsigned long long)n_f32);
    atomicAdd(g.counters + 2, (unsigned long long)n_f64);
    atomicAdd(g.counters + 3, (unsigned long long)n_blk);
  }
  return done || rlast >= rmax;
}

// stage 0: cell shells 0 .. 4 (occupied cells only: work-efficient while the neighbourhood is a few cells wide); stage 1: superblock
// shells -- blocks as cells, those beyond the current k-th distance skipped -- until the bound is met or the box is exhausted
template <int KMAX, bool FULL = false, bool FLAT = false>
__device__ __forceinline__ void knn_query_any(const SearchView& g, double qx, double qy, double qz, int want, TopK<KMAX, FULL>& top, bool skip_fine = false, int2* rl = nullptr,
                                              bool* sparse = nullptr) {
  if (g.binned) {
    const int k = top.k;
    const double bound = top.worst();  // the caller's max_sq_dist (nothing has been pushed yet)
    // (skip_fine: the row-tiled pass has scanned the shells 0 and 1 of the finest level, which therefore cannot settle the query; the
    // walk still starts there -- the list is not carried over -- but goes on to shell 4 at once)
    if constexpr (KMAX == 1) {
      if (knn_query_octant<KMAX, FULL>(g.bins[0], qx, qy, qz, top)) return;
    }
    bool settled = false;
    for (int l = 0; l < g.binned && !settled; l++) {
      if (l > 0) top.init(k, bound);
      settled = knn_query_bins<KMAX, FULL, FLAT>(g.bins[l], qx, qy, qz, top, (l + 1 < g.binned && !skip_fine) ? 1 : g.fine_shells, rl, (l + 1 == g.binned) ? sparse : nullptr);
      if (sparse && *sparse) return;
    }
    if (settled) return;
    if (sparse) {  // round 5: what the fine shells do not settle is searched by a whole wave (covariance_far_kernel), not by this lane with 63 others waiting
      *sparse = true;
      return;
    }
    // round 4: sparse neighbourhoods (the far field of a LiDAR scan: one point per cell) first try the BLOCKS as cells -- shells 0 .. block_stage of a grid four
    // times as coarse, 27 entries for the first two, a few points each -- before they start over on the superblocks, whose first shell alone scans every point
    // within 4-12 m of the query: those queries were the launch's tail (a hundred 64-query chunks of 350-460 us in a launch whose balanced length was 334 us)
    if (g.block_stage > 0) {
      top.init(k, bound);
      settled = knn_query_coarse<KMAX, false, FULL>(g.bins[g.binned - 1], qx, qy, qz, top, g.block_stage);
    }
    if (settled) return;
    top.init(k, bound);
    knn_query_coarse<KMAX, true, FULL>(g.bins[g.binned - 1], qx, qy, qz, top, 0x3fffffff);
  } else {
    knn_query_multi<KMAX, FULL>(g.hashed, qx, qy, qz, want, top);
  }
}

}  // namespace gp
