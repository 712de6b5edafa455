// gp_covariance_far.hpp -- the cooperative search of the covariance estimator for the queries with sparse neighbourhoods (covariance_far_kernel): sixteen lanes
// share one query of the list that gp_covariance.hip's covariance_kernel left behind.  A part of gp_covariance.hip, which launches it behind the per-lane search.
//
// Replaces (reference, CPU only): the k-NN loop of features/covariance_estimation.cpp:18-53 for the queries it is handed.
#pragma once

#include "gp_covariance_point.hpp"

namespace gp {

// ---- sparse neighbourhoods: SIXTEEN LANES PER QUERY (round 5) ----------------------------------------------------------------------
// A query the fine shells do not settle (the far field of a LiDAR scan: ring spacing of a metre, one point per 0.25 m cell) used to go on lane by lane: blocks as cells,
// then superblocks -- a chain of dependent loads on ONE lane while 63 wait: 400-600 us per wave against a mean of 110 (profiles/r05_c5_wavelog.txt), the tail of the
// launch.  Here kFarLanes lanes share one query (four queries per wave).  Such queries are few (0.1-1.5 % of a cloud), so the kernel runs at a fraction of a wave per
// SIMD and nothing hides a load's latency: what counts is the NUMBER OF DEPENDENT ROUND TRIPS, and every stage asks for everything it needs at once.
//   blocks -> candidates (far_process): a list of <= 128 blocks (4 x 4 x 4 cells: 1 m for the covariance structure), eight per lane: the eight block entries in one
//            trip, the sixteen cell_start words in the next, the (first point, length) ranges into LDS; then the CANDIDATES -- not the blocks -- are dealt to the lanes
//            (candidate o of the concatenated ranges to lane o % 16: one dense block does not leave fifteen lanes idle), eight loads in flight per lane;
//   phase A  the 5 x 5 x 5 blocks around the query's block: one list;
//   phase B  cube shells of SUPERBLOCKS (4 x 4 x 4 blocks, one 64-bit occupancy mask each) around the query's superblock, the masks dealt to the lanes four at a time:
//            empty space costs one 8-byte load per 64 m^3; occupied blocks outside phase A's cube and not farther than the group's best k-th distance so far are
//            appended to the list (LDS counter), which is processed whenever it is full and at the end of the shell.
// Every lane keeps the k best of what it scanned (exact f64 distances, strict '<' like KnnResult::push).  After phase A / a shell the group is done when k of its
// candidates lie within the safe radius (R units + the distance to the nearest face of the query's own unit: every unvisited point is farther) -- the stopping rule of the
// per-lane search, counted with ballots instead of read off a merged list -- or when the grid is exhausted.  Then the group merges its lists once: k rounds of "smallest
// head" (a group-wide minimum each; ties: smaller original index), which yields the neighbours in ascending order, the order covariance_from_neighbours sums them in.
// Exact like the per-lane search: the neighbour set is the k smallest distances either way.
constexpr int kFarBlockShells = 2, kFarLanes = 16, kFarList = 128, kFarPer = kFarList / kFarLanes, kFarMasks = 4;
struct FarGroupLds {
  int2 range[kFarList];  // (first point, points) per listed block
  int blk[kFarList];     // linear block index (phase B)
  int count;
  int pad_[3];
};
template <int KMAX, bool NORMALS = false>
// (four waves per SIMD = 128 registers, 560 B of scratch per lane: uncapped -- 256 registers, no scratch -- the kernel is 20 % faster ALONE (190 vs 240 us), but beside the
// other launch, whose waves hold a quarter of a SIMD's registers each, a 256-register wave waits until two of them on one SIMD have retired: profiles/r05_c5_summary.txt)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) covariance_far_kernel(BinGridView g, const float* __restrict__ points, int k, float* __restrict__ covs, int* __restrict__ num_short,
                                                             const int* __restrict__ far_list, const float* __restrict__ far_bound, const int* __restrict__ far_count,
                                                             float* __restrict__ normals = nullptr) {
  constexpr int kGroups = 64 / kFarLanes;
  // these few waves are chains of dependent round trips with short bursts of arithmetic in between, and they run beside the other launch's waves (four per SIMD, busy
  // with list insertions): at equal issue priority every burst takes four times as long -- the kernel measured 350 us beside the light queries' launch, 190 alone
  __builtin_amdgcn_s_setprio(3);
  __shared__ FarGroupLds lds_all[kGroups];  // (one wave per workgroup: a 256-register wave finds a place where a four-wave workgroup waits for four at once)
  const int lane = threadIdx.x & 63, sub = lane % kFarLanes, grp = lane / kFarLanes;
  FarGroupLds& L = lds_all[grp];
  const unsigned long long gmask = ((1ull << kFarLanes) - 1ull) << (grp * kFarLanes);
  const int groups = (int)gridDim.x * kGroups, count = *far_count;
  constexpr double kInf = 1.7976931348623157e308;
  auto wave_sync = [] {  // LDS traffic of a wave is ordered; this keeps the compiler from moving LDS accesses across it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  for (int w0 = (int)blockIdx.x * kGroups; w0 < count; w0 += groups) {  // (wave-uniform trip count; a group without a query idles through it)
    const int w = w0 + grp;
    const bool active = w < count;
    const int t = far_list[active ? w : w0];
    // what the per-lane search knew when it gave up: its k-th distance (rounded up; +inf when it had found fewer than k) -- nothing farther can be a neighbour, so
    // blocks beyond it are not even listed (a noise point a metre above a dense surface: without it phase A scanned 6000-8000 candidates, profiles/r05_c5_farlog.txt)
    const double known = (double)far_bound[active ? w : w0];
    double bound = known;  // nothing farther than this can be a neighbour: what the per-lane search knew, then the group's exact k-th distance after every stage
    const float4 self = g.sorted[t];
    const int i = __float_as_int(self.w);
    const double qx = (double)self.x, qy = (double)self.y, qz = (double)self.z;
    const double B = 4.0 * g.h, inv_B = 0.25 * g.inv_h;
    // block coordinates RELATIVE to the grid's first block (what the superblock masks are indexed by); the query is a point of the cloud: inside the grid
    const double ux = qx * inv_B - (double)g.geom.lo[0], uy = qy * inv_B - (double)g.geom.lo[1], uz = qz * inv_B - (double)g.geom.lo[2];
    const int c[3] = {fast_floor(ux), fast_floor(uy), fast_floor(uz)};
    const double fx = ux - (double)c[0], fy = uy - (double)c[1], fz = uz - (double)c[2];
    const double face = fmin(fmin(fmin(fx, 1.0 - fx), fmin(fy, 1.0 - fy)), fmin(fz, 1.0 - fz)) * B;
    const int dim[3] = {g.geom.dim[0], g.geom.dim[1], g.geom.dim[2]};
    const double ox = (double)g.geom.lo[0] * B, oy = (double)g.geom.lo[1] * B, oz = (double)g.geom.lo[2] * B;  // corner of block (0, 0, 0)
    TopK<KMAX, false> top;
    top.init(k, kInf);
    // the blocks listed for this group (nb <= kFarList; block index of list position j from `block_of(j)`) -> their points through the lanes' lists.
    // Wave-convergent: every lane of the wave calls it, groups without work pass nb = 0
    int fresh = 0;  // candidates the group has scanned since its lists were last merged (group-uniform)
    auto far_process = [&](int nb, auto block_of, auto block_wanted) {
      if (__builtin_amdgcn_ballot_w64(nb > 0) == 0ull) return;  // (an empty shell -- an outlier walks several: no round trips for nothing)
      int4 raw[kFarPer];
      bool wanted[kFarPer];
#pragma unroll
      for (int q = 0; q < kFarPer; q++) {
        const int j = sub * kFarPer + q;
        wanted[q] = j < nb && block_wanted(j);
        raw[q] = *reinterpret_cast<const int4*>(g.blocks + (wanted[q] ? block_of(j) : 0));  // (unconditional: the eight loads are in flight together)
      }
      int pb[kFarPer], pe[kFarPer];
#pragma unroll
      for (int q = 0; q < kFarPer; q++) {
        const unsigned long long bits = ((unsigned long long)(unsigned)raw[q].y << 32) | (unsigned long long)(unsigned)raw[q].x;
        const bool valid = wanted[q] && bits != 0ull;
        pb[q] = g.cell_start[valid ? raw[q].z : 0];
        pe[q] = valid ? g.cell_start[raw[q].z + __popcll(bits)] : pb[q];
      }
      int mine = 0;
#pragma unroll
      for (int q = 0; q < kFarPer; q++) {
        const int len = wanted[q] ? pe[q] - pb[q] : 0;
        L.range[sub * kFarPer + q] = make_int2(pb[q], len);
        mine += len;
      }
      int total = mine;
#pragma unroll
      for (int off = kFarLanes / 2; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
      wave_sync();
      fresh += total;
      // candidate o of the concatenated ranges -> lane o % kFarLanes; a lane's ordinals ascend, so its cursor over the ranges only moves forward
      int rj = 0, rc = 0;  // range under the cursor, candidates in front of it
      int2 cur = L.range[0];
      constexpr int kFarCand = 4;  // candidates in flight per lane
      for (int o = sub; __builtin_amdgcn_ballot_w64(o < total) != 0ull; o += kFarLanes * kFarCand) {
        int pp[kFarCand];
        bool ok[kFarCand];
#pragma unroll
        for (int q = 0; q < kFarCand; q++) {
          const int oq = o + q * kFarLanes;
          ok[q] = oq < total;
          if (ok[q]) {
            while (oq >= rc + cur.y) {
              rc += cur.y;
              rj++;
              cur = L.range[rj];
            }
            pp[q] = cur.x + (oq - rc);
          } else {
            pp[q] = 0;
          }
        }
        float4 v[kFarCand];
#pragma unroll
        for (int q = 0; q < kFarCand; q++) v[q] = g.sorted[pp[q]];
#pragma unroll
        for (int q = 0; q < kFarCand; q++)
          if (ok[q]) {
            const double ex = (double)v[q].x - qx, ey = (double)v[q].y - qy, ez = (double)v[q].z - qz;
            const double d2 = ex * ex + ey * ey + ez * ez;
            if (d2 <= bound) top.push(__float_as_int(v[q].w), d2);
          }
      }
      // a lane that holds k candidates bounds the group's k-th distance with its own (its list is a subset of the group's): `bound` tightens after EVERY list, without a
      // merge, and prunes the rest of the shell (the kitti scan's far kernel 230 -> 192 us; profiles/r05_c5_summary.txt item 6)
      double lane_kth = top.worst();
#pragma unroll
      for (int off = kFarLanes / 2; off > 0; off >>= 1) lane_kth = fmin(lane_kth, __shfl_xor(lane_kth, off, 64));
      bound = fmin(bound, lane_kth);
      wave_sync();  // (the list may be refilled)
    };
    // k candidates of the group within `safe`?  (a lane holds its k best: one that has k within the radius settles it alone)
    auto settled_within = [&](double safe, bool live) {
      const double safe2 = safe * safe;
      int within = 0;
#pragma unroll
      for (int j = 0; j < KMAX; j++) within += __popcll(__builtin_amdgcn_ballot_w64(live && j < k && top.idx[j] >= 0 && top.d[j] <= safe2) & gmask);
      return within >= k;
    };
    // the k smallest of the group's lists, ascending (ties: smaller index): k rounds of "smallest head", a group-wide minimum each -> fin.idx (group-uniform), the
    // group's exact k-th distance in `kth` (+inf while it holds fewer than k); returns how many there are.  ~4 us: once per shell, not per block
    int fin_i[KMAX];
    double kth = kInf;
    auto merge = [&]() -> int {
#pragma unroll
      for (int r = 0; r < KMAX; r++) fin_i[r] = -1;
      kth = kInf;
      int head = 0, n_have = 0;
#pragma unroll
      for (int r = 0; r < KMAX; r++) {
        double cur = kInf;
        int cur_i = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < KMAX; j++)
          if (head == j && j < k && top.idx[j] >= 0) cur = top.d[j], cur_i = top.idx[j];
        double m = cur;
#pragma unroll
        for (int off = kFarLanes / 2; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off, 64));
        int mi = cur == m ? cur_i : 0x7fffffff;
#pragma unroll
        for (int off = kFarLanes / 2; off > 0; off >>= 1) mi = min(mi, __shfl_xor(mi, off, 64));
        if (r < k && mi != 0x7fffffff) {
          fin_i[r] = mi;
          n_have = r + 1;
          if (r == k - 1) kth = m;
          if (cur == m && cur_i == mi) head++;  // (every candidate was scanned by exactly one lane: one winner)
        }
      }
      return n_have;
    };
    int have = 0;
    bool done = !active;
    auto box2 = [&](int bx, int by, int bz) {  // squared distance of a block's box from the query
      const double bx0 = ox + (double)bx * B, by0 = oy + (double)by * B, bz0 = oz + (double)bz * B;
      const double ddx = fmax(fmax(bx0 - qx, qx - (bx0 + B)), 0.0), ddy = fmax(fmax(by0 - qy, qy - (by0 + B)), 0.0), ddz = fmax(fmax(bz0 - qz, qz - (bz0 + B)), 0.0);
      return ddx * ddx + ddy * ddy + ddz * ddz;
    };
    // ---- phase A: the blocks around the query's block: the 3 x 3 x 3 cube, then -- with the bound that brought -- the shell around it.  One list each ----
    {
      int ra_max = 0;
#pragma unroll
      for (int a = 0; a < 3; a++) ra_max = max(ra_max, max(c[a], dim[a] - 1 - c[a]));  // the shell that covers the grid
      static_assert((2 * kFarBlockShells + 1) * (2 * kFarBlockShells + 1) * (2 * kFarBlockShells + 1) <= kFarList, "a cube of phase A is one list");
      for (int R = 1; R <= kFarBlockShells; R++) {
        const int x0 = max(c[0] - R, 0), x1 = min(c[0] + R, dim[0] - 1), y0 = max(c[1] - R, 0), y1 = min(c[1] + R, dim[1] - 1), z0 = max(c[2] - R, 0), z1 = min(c[2] + R, dim[2] - 1);
        const int nx = x1 - x0 + 1, ny = y1 - y0 + 1, nz = z1 - z0 + 1;
        far_process(
          done ? 0 : nx * ny * nz, [&](int j) { return ((size_t)(z0 + j / (nx * ny)) * (size_t)dim[1] + (size_t)(y0 + (j / nx) % ny)) * (size_t)dim[0] + (size_t)(x0 + j % nx); },
          [&](int j) {
            const int bx = x0 + j % nx, by = y0 + (j / nx) % ny, bz = z0 + j / (nx * ny);
            return (R == 1 || max(max(abs(bx - c[0]), abs(by - c[1])), abs(bz - c[2])) == R) && box2(bx, by, bz) <= bound;  // (not the cube of the step before)
          });
        const bool ok = settled_within((double)R * B + face, !done);
        if (!done && (ok || R >= ra_max)) done = true;
        if (__builtin_amdgcn_ballot_w64(!done && fresh > 0) != 0ull) {  // somebody goes on with new candidates: the exact k-th distance so far prunes what follows
          have = merge();
          bound = fmin(bound, kth);
          fresh = 0;
        }
      }
    }
    // ---- phase B: shells of superblocks (blocks outside phase A's cube) ----
    if (__builtin_amdgcn_ballot_w64(!done) != 0ull) {
      const double S = 4.0 * B;
      const int cs[3] = {c[0] >> 2, c[1] >> 2, c[2] >> 2};
      const double fsx = (ux - 4.0 * (double)cs[0]) * 0.25, fsy = (uy - 4.0 * (double)cs[1]) * 0.25, fsz = (uz - 4.0 * (double)cs[2]) * 0.25;
      const double sface = fmin(fmin(fmin(fsx, 1.0 - fsx), fmin(fsy, 1.0 - fsy)), fmin(fsz, 1.0 - fsz)) * S;
      int rs_max = 0;
#pragma unroll
      for (int a = 0; a < 3; a++) rs_max = max(rs_max, max(cs[a], g.sdim[a] - 1 - cs[a]));
      for (int R = 0; __builtin_amdgcn_ballot_w64(!done) != 0ull; R++) {  // (the wave goes on while any of its groups does; a group ends at rs_max at the latest)
        // the SURFACE of the cube of radius R, enumerated directly (an outlier tens of metres from everything walks six shells: the cube's 2197 positions at R = 6 are
        // 866 on the surface): the two z-faces, (2R + 1)^2 positions each, then 2R - 1 slabs with the 8R positions of their rim
        const int side = 2 * R + 1, face_n = side * side, rim_n = 8 * R;
        const int total = done ? 0 : (R == 0 ? 1 : 2 * face_n + (side - 2) * rim_n);
        auto shell_pos = [&](int e, int& dx, int& dy, int& dz) {
          if (R == 0) {
            dx = dy = dz = 0;
          } else if (e < 2 * face_n) {
            const int f = e / face_n, r = e % face_n;
            dz = f ? R : -R;
            dx = r % side - R;
            dy = r / side - R;
          } else {
            const int r = e - 2 * face_n, slab = r / rim_n, pos = r % rim_n, edge = pos / (2 * R), off = pos % (2 * R);
            dz = slab - R + 1;
            dx = edge == 0 ? -R + off : (edge == 1 ? R : (edge == 2 ? R - off : -R));
            dy = edge == 0 ? -R : (edge == 1 ? -R + off : (edge == 2 ? R : R - off));
          }
        };
        int e = sub;                        // next position of the shell this lane looks at (stride kFarLanes)
        unsigned long long rest[kFarMasks];  // occupied blocks of the lane's current masks that are still to be listed
        unsigned long long spos[kFarMasks];  // their superblocks, packed (x | y << 21 | z << 42: a grid has < 2^24 blocks)
#pragma unroll
        for (int q = 0; q < kFarMasks; q++) rest[q] = 0ull, spos[q] = 0;
        bool lane_more = e < total;
        while (__builtin_amdgcn_ballot_w64(lane_more) != 0ull) {  // rounds of: fill the group's list (<= kFarList blocks), process it
          // (`bound`: the group's exact k-th distance as of the last stage -- a block farther away than that holds nothing of interest)
          if (sub == 0) L.count = 0;
          wave_sync();
          bool full = false;
          while (lane_more && !full) {
            bool any_rest = false;
#pragma unroll
            for (int q = 0; q < kFarMasks; q++) any_rest = any_rest || rest[q] != 0ull;
            if (!any_rest) {  // the next kFarMasks masks of this lane's positions, requested together
              if (e >= total) {
                lane_more = false;
                break;
              }
#pragma unroll
              for (int q = 0; q < kFarMasks; q++) {
                const int eq = e + q * kFarLanes;
                int dx = 0, dy = 0, dz = 0;
                shell_pos(eq < total ? eq : 0, dx, dy, dz);
                const int x = cs[0] + dx, y = cs[1] + dy, z = cs[2] + dz;
                const bool in = eq < total && x >= 0 && x < g.sdim[0] && y >= 0 && y < g.sdim[1] && z >= 0 && z < g.sdim[2];
                const unsigned long long mask = g.super[in ? ((size_t)z * (size_t)g.sdim[1] + (size_t)y) * (size_t)g.sdim[0] + (size_t)x : 0];
                rest[q] = in ? mask : 0ull;
                spos[q] = (unsigned long long)(unsigned)x | ((unsigned long long)(unsigned)y << 21) | ((unsigned long long)(unsigned)z << 42);
              }
              e += kFarMasks * kFarLanes;
            }
#pragma unroll
            for (int q = 0; q < kFarMasks; q++) {
              while (rest[q] != 0ull && !full) {
                const int bit = __ffsll((long long)rest[q]) - 1;
                const int bx = 4 * (int)(spos[q] & 0x1fffffull) + (bit & 3), by = 4 * (int)((spos[q] >> 21) & 0x1fffffull) + ((bit >> 2) & 3), bz = 4 * (int)(spos[q] >> 42) + (bit >> 4);
                bool want = max(max(abs(bx - c[0]), abs(by - c[1])), abs(bz - c[2])) > kFarBlockShells;  // (else: phase A scanned it)
                if (want) want = box2(bx, by, bz) <= bound;
                if (want) {
                  const int slot = atomicAdd(&L.count, 1);
                  if (slot >= kFarList) {  // the list is full: this block waits for the next round
                    full = true;
                    break;
                  }
                  L.blk[slot] = (bz * dim[1] + by) * dim[0] + bx;
                }
                rest[q] &= rest[q] - 1ull;
              }
            }
          }
          wave_sync();
          const int nb = done ? 0 : min(L.count, kFarList);
          wave_sync();
          // (Scanning an unbounded group's nearest blocks first -- eight at a time until it holds k candidates, the rest against that bound -- cuts an outlier's candidates
          // from 1500 to 350 per lane and not its time: the 160-260 us of such a query are the ~35 dependent mask trips of five empty shells, not the surface behind them.
          // Measured and removed: profiles/r05_c5_summary.txt item 7.)
          far_process(nb, [&](int j) { return (size_t)L.blk[j]; }, [](int) { return true; });
        }
        const bool ok = settled_within((double)R * S + sface, !done);
        if (!done && (ok || R >= rs_max)) done = true;
        if (__builtin_amdgcn_ballot_w64(!done && fresh > 0) != 0ull) {  // (a shell that brought nothing leaves the bound as it is: no merge)
          have = merge();
          bound = fmin(bound, kth);
          fresh = 0;
        }
      }
    }
    // ---- the k smallest of the group's lists, ascending (ties: smaller index) ----
    have = merge();
    if (active && sub == 0) {
      float* out = (!NORMALS || covs) ? covs + 9 * (size_t)i : nullptr;
      float* nout = NORMALS ? normals + 3 * (size_t)i : nullptr;
      if (have < k) {
        atomicAdd(num_short, 1);
        store_identity<NORMALS>(self.x, out, nout);
      } else {
        TopK<KMAX, false> fin;
        fin.init(k, kInf);
#pragma unroll
        for (int r = 0; r < KMAX; r++) fin.idx[r] = fin_i[r];
        covariance_from_neighbours<KMAX, false, NORMALS>(fin, points, k, out, nout, qx, qy, qz);
      }
    }
  }
}

}  // namespace gp
