// gp_xyzi_search.hpp -- the device side of the exact nearest-neighbour search in (x, y, z, intensity) space: the walkers over the structures of gp_knn_grid.hpp
// with a cell-sorted copy of the target's intensities beside their cell-sorted points.  Device code only, no kernels: gp_intensity_search.hip calls it.
//
// Replaces (reference, CPU only -- there is no GPU counterpart upstream):
//   ann/intensity_kdtree.hpp:41-47, src/gtsam_points/ann/intensity_kdtree.cpp:21-32     IntensityKdTree::knn_search, k = 1
//
// The metric is the reference's AS WRITTEN: d4^2(j) = |q - x_j|^2 + (I_q - s I_j)^2 with the scale s on the STORED side only (kdtree_get_pt multiplies by
// intensity_scale, the factors put the raw source intensity into pt[3]).  Distances are formed in f64 on the f32 inputs, s I_j as one f64 product.
//
// Exactness: the walk is gp_knn_search.hpp's shell walk over the 3-D cells.  After shell r every unvisited point j has |q - x_j| >= d_safe(r) = r h + (distance from
// the query to the nearest face of its own cell), and d4^2(j) >= |q - x_j|^2, so a 4-D best distance below d_safe(r)^2 cannot be beaten: the 3-D stop rule stays
// exact as long as the list's worst distance is the 4-D one.  (It stops later than a 3-D search would: candidates near in space and far in intensity do not end it.)
// The stop is strict (best < d_safe^2) and a candidate replaces the held one when it is nearer or equally near with a lower index, so the result is the LOWEST
// INDEX among the nearest, whatever order the cells and the points inside a cell are visited in (the hashed grid's cells are filled by atomics).
// A candidate is held only when its distance is strictly below the caller's cut-off; a non-finite distance (a non-finite target coordinate or intensity) is never held.
#pragma once

#include "gp_knn_search.hpp"

namespace gp {

struct XyziBest {
  double d;  // the caller's cut-off while nothing is held
  int idx;
  __device__ __forceinline__ void init(double max_sq_dist) {
    d = max_sq_dist;
    idx = -1;
  }
  __device__ __forceinline__ void push(int index, double dist) {
    if (dist < d || (dist == d && idx >= 0 && index < idx)) {
      d = dist;
      idx = index;
    }
  }
};

// what a 4-D search runs on: the 3-D structure and, per level of it that is walked, the intensities in the order of that level's `sorted`
struct XyziView {
  SearchView grid;
  const float* sorted_intensities[kMaxLevels];  // binned: [0] beside bins[0].sorted; hashed: [l] beside hashed.lv[l].sorted
  double scale;
};

__device__ __forceinline__ double xyzi_sq_dist(const float4 v, float stored, double scale, double qx, double qy, double qz, double qi) {
  const double ddx = (double)v.x - qx, ddy = (double)v.y - qy, ddz = (double)v.z - qz, ddi = qi - scale * (double)stored;
  return (ddx * ddx + ddy * ddy + ddz * ddz) + ddi * ddi;
}

// the candidates [pb, pe) of one cell, four loads of each array in flight (the clamped repeats of the last point cannot displace it: same index, same distance)
__device__ __forceinline__ void xyzi_scan_range(const float4* __restrict__ sorted, const float* __restrict__ sint, double scale, int pb, int pe, double qx, double qy,
                                                double qz, double qi, XyziBest& best) {
  const int last = pe - 1;
  for (int p = pb; p < pe; p += 4) {
    const int p1 = min(p + 1, last), p2 = min(p + 2, last), p3 = min(p + 3, last);
    const float4 v0 = sorted[p], v1 = sorted[p1], v2 = sorted[p2], v3 = sorted[p3];
    const float i0 = sint[p], i1 = sint[p1], i2 = sint[p2], i3 = sint[p3];
    best.push(__float_as_int(v0.w), xyzi_sq_dist(v0, i0, scale, qx, qy, qz, qi));
    best.push(__float_as_int(v1.w), xyzi_sq_dist(v1, i1, scale, qx, qy, qz, qi));
    best.push(__float_as_int(v2.w), xyzi_sq_dist(v2, i2, scale, qx, qy, qz, qi));
    best.push(__float_as_int(v3.w), xyzi_sq_dist(v3, i3, scale, qx, qy, qz, qi));
  }
}

// The binned structure: cube shells of cells around the query's cell, one 16-B block entry per 4 x 4 x 4 cells, occupied cells only (knn_query_bins' walk without its
// candidate list and its f32 filter -- every candidate costs its f64 distance here).  A cell whose box lies farther from the query than the held 4-D distance is skipped:
// its points' 3-D distances alone exceed it.
__device__ __forceinline__ void xyzi_query_bins(const BinGridView& g, const float* __restrict__ sint, double scale, double qx, double qy, double qz, double qi, XyziBest& best) {
  const double ux = qx * g.inv_h, uy = qy * g.inv_h, uz = qz * g.inv_h;
  if (!cell_in_range(ux, uy, uz)) return;  // non-finite query: no neighbour
  const int c[3] = {fast_floor(ux), fast_floor(uy), fast_floor(uz)};
  const double f[3] = {ux - (double)c[0], uy - (double)c[1], uz - (double)c[2]};
  const double face = fmin(fmin(fmin(f[0], 1.0 - f[0]), fmin(f[1], 1.0 - f[1])), fmin(f[2], 1.0 - f[2])) * g.h;
  const double h2 = g.h * g.h * 0.9999;  // (the box test only ever skips, with slack for its own rounding)
  int lo[3], hi[3], r0 = 0, rmax = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = g.geom.lo[a] * 4;
    hi[a] = (g.geom.lo[a] + g.geom.dim[a]) * 4 - 1;
    r0 = max(r0, max(lo[a] - c[a], c[a] - hi[a]));              // first shell that reaches the box
    rmax = max(rmax, max(abs(c[a] - lo[a]), abs(c[a] - hi[a])));  // shell that covers it
  }
  for (int r = r0; r <= rmax; r++) {
    int b0[3], b1[3];
    bool any = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const int x0 = max(c[a] - r, lo[a]), x1 = min(c[a] + r, hi[a]);
      any = any && x0 <= x1;
      b0[a] = x0 >> 2;
      b1[a] = x1 >> 2;
    }
    if (any) {
      // only blocks that touch the shell: a z-slab inside the previous cube along z contributes its y-border rows, such a row its two x-border blocks
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
            const unsigned long long bits = ((unsigned long long)(unsigned)raw.y << 32) | (unsigned long long)(unsigned)raw.x;
            if (bits == 0ull) continue;
            unsigned long long m = bits & cube_mask(mx, my, mz) & ~cube_mask(mx1, my1, mz1);  // occupied cells of this shell
            while (m) {
              const int bit = __ffsll((long long)m) - 1;
              m &= m - 1ull;
              if (r > 0) {
                const double rx = (double)(4 * bx + (bit & 3) - c[0]) - f[0], ry = (double)(4 * by + ((bit >> 2) & 3) - c[1]) - f[1],
                             rz = (double)(4 * bz + (bit >> 4) - c[2]) - f[2];
                const double ex = fmax(fmax(rx, -rx - 1.0), 0.0), ey = fmax(fmax(ry, -ry - 1.0), 0.0), ez = fmax(fmax(rz, -rz - 1.0), 0.0);
                if ((ex * ex + ey * ey + ez * ez) * h2 > best.d) continue;
              }
              const int ord = raw.z + __popcll(bits & ((1ull << bit) - 1ull));
              xyzi_scan_range(g.sorted, sint, scale, g.cell_start[ord], g.cell_start[ord + 1], qx, qy, qz, qi, best);
            }
          }
        }
      }
    }
    const double safe = (double)r * g.h + face;
    if (best.d < safe * safe) return;  // every unvisited point is farther in 3-D, hence in 4-D, than the held one (or than the cut-off)
  }
}

// The hashed grid (clouds whose bounding box is too large for the block grid): knn_query's walk on one level.
__device__ __forceinline__ void xyzi_query_hashed(const GridView& g, const float* __restrict__ sint, double scale, double qx, double qy, double qz, double qi, XyziBest& best) {
  if (!(fabs(qx) < 1.0e300 && fabs(qy) < 1.0e300 && fabs(qz) < 1.0e300)) return;  // non-finite query: no neighbour
  const int cx = hashed_cell(qx * g.inv_h), cy = hashed_cell(qy * g.inv_h), cz = hashed_cell(qz * g.inv_h);
  const double fx = qx * g.inv_h - (double)cx, fy = qy * g.inv_h - (double)cy, fz = qz * g.inv_h - (double)cz;
  const double face = fmin(fmin(fmin(fx, 1.0 - fx), fmin(fy, 1.0 - fy)), fmin(fz, 1.0 - fz)) * g.h;
  const int rmax = max(max(max(abs(cx - g.lo[0]), abs(cx - g.hi[0])), max(abs(cy - g.lo[1]), abs(cy - g.hi[1]))), max(abs(cz - g.lo[2]), abs(cz - g.hi[2])));
  for (int r = 0; r <= rmax; r++) {
    for (int dz = -r; dz <= r; dz++)
      for (int dy = -r; dy <= r; dy++) {
        const bool shell_yz = (dz == -r || dz == r || dy == -r || dy == r);
        const int step = (shell_yz || r == 0) ? 1 : 2 * r;  // interior rows: only dx = -r and dx = +r belong to the shell
        for (int dx = -r; dx <= r; dx += step) {
          const int s = grid_find(g, pack_cell(cx + dx, cy + dy, cz + dz));
          if (s < 0) continue;
          xyzi_scan_range(g.sorted, sint, scale, g.start[s], g.start[s + 1], qx, qy, qz, qi, best);
        }
      }
    const double safe = (double)r * g.h + face;
    if (best.d < safe * safe) return;
  }
}

// One query (q, I_q): the binned structure's finest level, or the level of the hashed grid knn_query_multi would pick for a 1-NN search (the finest whose 3 x 3 x 3
// neighbourhood holds two points; the choice affects speed only).  A non-finite query intensity finds nothing.
__device__ __forceinline__ void xyzi_query_any(const XyziView& v, double qx, double qy, double qz, double qi, XyziBest& best) {
  if (!(fabs(qi) < 1.0e300)) return;
  if (v.grid.binned) {
    xyzi_query_bins(v.grid.bins[0], v.sorted_intensities[0], v.scale, qx, qy, qz, qi, best);
  } else {
    const MultiGridView& mg = v.grid.hashed;
    int level = mg.num_levels - 1;
    for (int l = 0; l + 1 < mg.num_levels; l++) {
      if (count27(mg.lv[l], qx, qy, qz) >= 2) {
        level = l;
        break;
      }
    }
    xyzi_query_hashed(mg.lv[level], v.sorted_intensities[level], v.scale, qx, qy, qz, qi, best);
  }
}

}  // namespace gp
