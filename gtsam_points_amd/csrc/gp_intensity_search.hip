// gp_intensity_search.hip -- the exact nearest-neighbour search in (x, y, z, intensity) space: the structure (a gp_point_grid over the target's points and, beside its
// cell-sorted points, a cell-sorted copy of the target's intensities), the query entry point and the correspondence pass of the photometric factors
// (gp_color_consistency.hip; the colored GICP factor of gp_colored_factors.hip when it is handed this structure).  The walk is gp_xyzi_search.hpp.
//
// Replaces (reference, CPU only -- there is no GPU counterpart upstream):
//   ann/intensity_kdtree.hpp, src/gtsam_points/ann/intensity_kdtree.cpp                        IntensityKdTree (nanoflann, 4-D)   -> gp_intensity_grid_*
//   factors/impl/integrated_color_consistency_factor_impl.hpp:118-135, _colored_gicp_:116-129  update_correspondences on it       -> gp::launch_nearest_correspondences_xyzi
#include <cmath>
#include <cstring>
#include <memory>

#include "gp_xyzi_search.hpp"

// the structure: OWNS its 3-D grid and the intensity copies, BORROWS the target's arrays
struct gp_intensity_grid {
  gp_point_grid* grid = nullptr;
  gp::DeviceArray sorted_intensities[gp::kMaxLevels];
  const float* points = nullptr;
  const float* intensities = nullptr;
  int n = 0;
  double scale = 1.0;
  gp::XyziView view() const {
    gp::XyziView v{};
    v.grid = grid->view();
    for (int l = 0; l < gp::kMaxLevels; l++) v.sorted_intensities[l] = sorted_intensities[l].as<float>();
    v.scale = scale;
    return v;
  }
  ~gp_intensity_grid() {
    if (grid) gp_point_grid_destroy(grid);  // (synchronises the device: every search has finished with the copies below too)
  }
};

namespace gp {

// sorted_intensities[p] = the intensity of the point at position p of a level's cell-sorted points (whose w carries the original index): a candidate's intensity
// then comes with the same index as its position -- two independent loads -- instead of one more dependent round trip through the original index per candidate
__global__ void __launch_bounds__(256) gather_sorted_intensities_kernel(const float4* __restrict__ sorted, const float* __restrict__ intensities, int n,
                                                                        float* __restrict__ sorted_intensities) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  sorted_intensities[p] = intensities[(size_t)__float_as_int(sorted[p].w)];
}

// gp_intensity_grid_search: one query per lane, queries double[m][4] = (x, y, z, intensity)
__global__ void __launch_bounds__(256) xyzi_search_kernel(XyziView g, const double* __restrict__ queries, int m, double max_sq_dist, int* __restrict__ indices,
                                                          double* __restrict__ sq_dists) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const double* q = queries + 4 * (size_t)i;
  XyziBest best;
  best.init(max_sq_dist);
  xyzi_query_any(g, q[0], q[1], q[2], q[3], best);
  indices[i] = best.idx;
  if (sq_dists) sq_dists[i] = best.d;
}

struct NearestXyziDesc {
  const float* points;
  const float* intensities;
  XyziView grid;
  int n;
  double max_sq_dist;
  double pose[16];  // rides in the kernel arguments (no H2D copy in front of the launch)
};

// update_correspondences of the photometric factors on an IntensityKdTree: corr[i] = index of the target point nearest to (T p_i, I_i) in XYZI with squared 4-D
// distance < max, or -1.  ONE query per lane and nothing else in the kernel, for the reason recorded above nearest_correspond_kernel (gp_knn.hip).
__global__ void __launch_bounds__(256) nearest_correspond_xyzi_kernel(NearestXyziDesc f, int* __restrict__ corr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= f.n) return;
  const Pose Tl = load_pose(f.pose);
  const double px = (double)f.points[3 * (size_t)i], py = (double)f.points[3 * (size_t)i + 1], pz = (double)f.points[3 * (size_t)i + 2];
  const double lx = Tl.r00 * px + Tl.r01 * py + Tl.r02 * pz + Tl.tx;
  const double ly = Tl.r10 * px + Tl.r11 * py + Tl.r12 * pz + Tl.ty;
  const double lz = Tl.r20 * px + Tl.r21 * py + Tl.r22 * pz + Tl.tz;
  XyziBest best;
  best.init(f.max_sq_dist);
  xyzi_query_any(f.grid, lx, ly, lz, (double)f.intensities[i], best);
  corr[i] = best.idx;
}

int launch_nearest_correspondences_xyzi(const gp_intensity_grid* grid, const float* points, const float* intensities, int n, const double pose_lin[16], double max_sq_dist,
                                        int* corr, hipStream_t stream) {
  NearestXyziDesc f;
  f.points = points;
  f.intensities = intensities;
  f.grid = grid->view();
  f.n = n;
  f.max_sq_dist = max_sq_dist;
  memcpy(f.pose, pose_lin, sizeof(double) * 16);
  hipLaunchKernelGGL(nearest_correspond_xyzi_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, f, corr);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

}  // namespace gp

extern "C" {

int gp_intensity_grid_create(const float* points_dev, const float* intensities_dev, int n, double intensity_scale, double cell_size, gp_stream_t stream,
                             gp_intensity_grid_t** out) {
  if (!points_dev || !intensities_dev || n < 0 || !std::isfinite(intensity_scale) || !out)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_intensity_grid_create: bad arguments (a NULL array, a negative count, an intensity_scale that is not finite)");
  auto g = std::make_unique<gp_intensity_grid>();
  g->points = points_dev;
  g->intensities = intensities_dev;
  g->n = n;
  g->scale = intensity_scale;
  GP_TRY(gp_point_grid_create(points_dev, n, cell_size > 0.0 ? cell_size : 0.25, stream, &g->grid));
  hipStream_t s = (hipStream_t)stream;
  const gp::SearchView v = g->grid->view();
  // the levels the walk may read: the binned structure's finest, or every level of the hashed grid
  const int levels = v.binned ? 1 : v.hashed.num_levels;
  for (int l = 0; l < levels; l++) {
    const float4* sorted = v.binned ? v.bins[0].sorted : v.hashed.lv[l].sorted;
    const int count = v.binned ? v.bins[0].n : v.hashed.lv[l].n;
    GP_TRY(g->sorted_intensities[l].alloc_pooled(sizeof(float) * (size_t)std::max(count, 1), s));
    if (count > 0)
      hipLaunchKernelGGL(gp::gather_sorted_intensities_kernel, dim3((count + 255) / 256), dim3(256), 0, s, sorted, intensities_dev, count, g->sorted_intensities[l].as<float>());
  }
  GP_HIP(hipGetLastError());
  GP_HIP(hipStreamSynchronize(s));  // (a search takes a stream of its own, which need not be this one)
  *out = g.release();
  return GP_OK;
}

int gp_intensity_grid_destroy(gp_intensity_grid_t* g) {
  delete g;
  return GP_OK;
}

const gp_point_grid_t* gp_intensity_grid_point_grid(const gp_intensity_grid_t* g) { return g ? g->grid : nullptr; }

int gp_intensity_grid_search(const gp_intensity_grid_t* g, const double* queries_dev, int m, double max_sq_dist, int* indices_dev, double* sq_dists_dev, gp_stream_t stream) {
  if (!g || m < 0 || (m > 0 && (!queries_dev || !indices_dev))) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_intensity_grid_search: bad arguments (a NULL handle or array, m < 0)");
  if (m == 0) return GP_OK;
  hipLaunchKernelGGL(gp::xyzi_search_kernel, dim3((m + 255) / 256), dim3(256), 0, (hipStream_t)stream, g->view(), queries_dev, m, max_sq_dist, indices_dev, sq_dists_dev);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

}  // extern "C"
