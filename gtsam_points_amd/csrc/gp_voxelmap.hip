// gp_voxelmap.hip -- GaussianVoxelMapGPU for gfx950: the handle, the two builds and the two queries.
//
//   * gp_voxelmap_insert builds the map.  The DEFAULT is the binned build (insert_binned): gp_binning.hpp sorts the points by voxel, the statistics are an ordered
//     segmented sum without atomics, and the whole build waits for the device once.  The hashed build (insert_hashed) is the reference's own scheme -- buckets claimed
//     with atomicCAS, statistics accumulated with f64 atomics -- and runs for an empty cloud, for a cloud whose box exceeds the block grid, and under
//     GP_TUNE_MAP_BUILD (A/B, tests).  The kernels of both are in gp_voxelmap_kernels.hpp.
//   * gp_voxelmap_lookup / gp_voxelmap_overlap: lookup_kernel, below.
//   * the line table of the hashed VGICP kernel family (build_private_table / ensure_private_table).
// Download, assign, save / load, clone, offload / reload: gp_voxelmap_store.hip.
//
// Replaces src/gtsam_points/types/gaussian_voxelmap_gpu.cu (insert :211-251, create_bucket_table :253-307) and the overlap/lookup half of
// gaussian_voxelmap_gpu_funcs.cu:156-236.
#include "gp_scan.hpp"
#include "gp_voxelmap.hpp"
#include "gp_voxelmap_kernels.hpp"

namespace gp {

// voxel_bucket_assignment_kernel (gaussian_voxelmap_gpu.cu:37-75): claim a bucket per distinct voxel coordinate.
// rep[b] = index of the first point that claimed bucket b, or -1.
__global__ void __launch_bounds__(256) claim_buckets_kernel(const float* __restrict__ points, int n, int* __restrict__ rep, uint32_t num_buckets,
                                                            uint32_t mask, int max_scan, double inv_leaf, int* __restrict__ invalid,
                                                            int* __restrict__ failures) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int cx, cy, cz;
  if (!point_coord(points, i, inv_leaf, cx, cy, cz)) {  // neither a member nor a failure: counted apart, so that the drop rate is over the valid points
    atomicAdd(invalid, 1);
    return;
  }
  const uint64_t hash = coord_hash(cx, cy, cz);
  for (int j = 0; j < max_scan; j++) {
    const uint32_t b = bucket_index(hash, j, num_buckets, mask);
    const int old = atomicCAS(&rep[b], -1, i);
    if (old < 0) return;  // claimed an empty bucket
    int ox, oy, oz;
    point_coord(points, old, inv_leaf, ox, oy, oz);  // (a representative is a valid point: only those claim)
    if (ox == cx && oy == cy && oz == cz) return;  // voxel already present
  }
  atomicAdd(failures, 1);  // probe chain exhausted: this point is dropped (gaussian_voxelmap_gpu.cu:67)
}

// voxel_coord_select_kernel (:77-90) + voxel id allocation (:57-60)
__global__ void __launch_bounds__(256) assign_voxels_kernel(const float* __restrict__ points, const int* __restrict__ rep, uint32_t num_buckets,
                                                            double inv_leaf, gp_voxel_bucket* __restrict__ buckets, int* __restrict__ voxel_coords,
                                                            int* __restrict__ num_voxels) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= num_buckets) return;
  const int r = rep[b];
  int4 out = make_int4(0, 0, 0, -1);
  if (r >= 0) {
    int cx, cy, cz;
    point_coord(points, r, inv_leaf, cx, cy, cz);
    const int v = atomicAdd(num_voxels, 1);
    out = make_int4(cx, cy, cz, v);
    voxel_coords[3 * (size_t)v] = cx;
    voxel_coords[3 * (size_t)v + 1] = cy;
    voxel_coords[3 * (size_t)v + 2] = cz;
  }
  reinterpret_cast<int4*>(buckets)[b] = out;
}

// accumulate_points_kernel (:92-152): sums[v] = { sum(p - centre) (3), sum upper(C) (6) } in double, count, max intensity
__global__ void __launch_bounds__(256) accumulate_kernel(const float* __restrict__ points, const float* __restrict__ covs,
                                                         const float* __restrict__ intensities, int n, VoxelMapView map, double* __restrict__ sums,
                                                         int* __restrict__ counts, unsigned int* __restrict__ intensity_bits) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double px = (double)points[3 * (size_t)i], py = (double)points[3 * (size_t)i + 1], pz = (double)points[3 * (size_t)i + 2];
  int cx, cy, cz;
  if (!cell_of(px, py, pz, map.inv_leaf, cx, cy, cz)) return;  // NaN / inf / out of range: in no voxel
  const int v = lookup_voxel(map, cx, cy, cz);
  if (v < 0) return;  // dropped at table build
  double ox, oy, oz;
  voxel_center(map, cx, cy, cz, ox, oy, oz);
  const float* c = covs + 9 * (size_t)i;
  double* s = sums + 9 * (size_t)v;
  unsafeAtomicAdd(s + 0, px - ox);
  unsafeAtomicAdd(s + 1, py - oy);
  unsafeAtomicAdd(s + 2, pz - oz);
  unsafeAtomicAdd(s + 3, (double)c[0]);  // xx
  unsafeAtomicAdd(s + 4, 0.5 * ((double)c[3] + (double)c[1]));  // xy: symmetric part of the column-major 3x3 (the input itself when symmetric)
  unsafeAtomicAdd(s + 5, 0.5 * ((double)c[6] + (double)c[2]));  // xz
  unsafeAtomicAdd(s + 6, (double)c[4]);                         // yy
  unsafeAtomicAdd(s + 7, 0.5 * ((double)c[7] + (double)c[5]));  // yz
  unsafeAtomicAdd(s + 8, (double)c[8]);  // zz
  atomicAdd(counts + v, 1);
  if (intensities) {
    // intensity_max over the voxel, from +0.0: only x > 0 can change it, and among positive floats (inf included) the order of the bit patterns is the order of
    // the values -- atomicMax on the bits (:138-139) of those alone
    const float x = intensities[i];
    if (x > 0.0f) atomicMax(intensity_bits + v, __float_as_uint(x));
  }
}

// finalize_voxels_kernel (:154-172): divide by the count; emit the gather record, the means and the covariances (the counts, intensities and coordinates are in place)
__global__ void __launch_bounds__(256) finalize_kernel(int num_voxels, double leaf, const int* __restrict__ voxel_coords, const double* __restrict__ sums,
                                                       const int* __restrict__ counts, VoxelOutputs out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num_voxels) return;
  const int* c = voxel_coords + 3 * (size_t)v;
  emit_voxel_stats(out, v, counts[v], sums + 9 * (size_t)v, voxel_centre(c[0], leaf), voxel_centre(c[1], leaf), voxel_centre(c[2], leaf));
}

// line table: claim the first free key slot of the home line (front to back), else walk to the next line
__global__ void __launch_bounds__(256) line_claim_kernel(int num_voxels, const int* __restrict__ voxel_coords, gp_voxel_bucket* __restrict__ lines, uint32_t lmask) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num_voxels) return;
  const int cx = voxel_coords[3 * (size_t)v], cy = voxel_coords[3 * (size_t)v + 1], cz = voxel_coords[3 * (size_t)v + 2];
  uint32_t l = coord_hash32(cx, cy, cz) & lmask;
  for (;;) {
    gp_voxel_bucket* line = lines + 4 * (size_t)l;
    for (int t = 0; t < 4; t++) {
      if (atomicCAS(&line[t].voxel_index, -1, v) == -1) {
        line[t].coord[0] = cx;
        line[t].coord[1] = cy;
        line[t].coord[2] = cz;
        return;
      }
    }
    l = (l + 1) & lmask;
  }
}

// ---- occupancy-block grid (gp_device.hpp: GridBlock; geometry helpers in gp_binning.hpp) ----

// bounding box of the set's living voxels in block units: bbox[0..2] = min, bbox[3..5] = max (wave reduce + one atomic per wave; a lane without a living voxel
// contributes the empty box)
__global__ void __launch_bounds__(256) voxels_bbox_kernel(VoxelSet set, int* __restrict__ bbox) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const bool alive = set.alive(v);
  CellBox box;
  if (alive) {
    const int b[3] = {set.coords[3 * (size_t)v] >> 2, set.coords[3 * (size_t)v + 1] >> 2, set.coords[3 * (size_t)v + 2] >> 2};
    box.add(b);
  }
  box.wave_reduce();
  if ((threadIdx.x & 63) == 0 && !box.empty()) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      atomicMin(bbox + a, box.lo[a]);
      atomicMax(bbox + 3 + a, box.hi[a]);
    }
  }
}

// the set's living voxels mark their bits in the grid.  The box holds them by construction (a one-shot build's voxels; the survivors and the cells of an incremental
// insert); a coordinate outside it marks nothing
__global__ void __launch_bounds__(256) grid_mark_kernel(VoxelSet set, GridGeom g, GridBlock* __restrict__ blocks) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (!set.alive(v)) return;
  const int cx = set.coords[3 * (size_t)v], cy = set.coords[3 * (size_t)v + 1], cz = set.coords[3 * (size_t)v + 2];
  if (!grid_contains(g, cx, cy, cz)) return;
  atomicOr(&blocks[grid_block_index(g, cx, cy, cz)].bits, 1ull << grid_bit(cx, cy, cz));
}

__global__ void __launch_bounds__(256) grid_count_kernel(long long num_blocks, GridBlock* __restrict__ blocks) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < num_blocks) blocks[b].base = __popcll(blocks[b].bits);
}

// new index of every voxel = its ordinal in the grid; coordinates move to the new order
__global__ void __launch_bounds__(256) grid_renumber_kernel(int num_voxels, const int* __restrict__ coords_old, GridGeom g, const GridBlock* __restrict__ blocks,
                                                            int* __restrict__ perm, int* __restrict__ coords_new) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num_voxels) return;
  const int cx = coords_old[3 * (size_t)v], cy = coords_old[3 * (size_t)v + 1], cz = coords_old[3 * (size_t)v + 2];
  const int nv = grid_ordinal(g, blocks, cx, cy, cz);
  if (nv < 0) return;  // (cannot happen: its bit was marked from this very list)
  perm[v] = nv;
  coords_new[3 * (size_t)nv] = cx;
  coords_new[3 * (size_t)nv + 1] = cy;
  coords_new[3 * (size_t)nv + 2] = cz;
}


__global__ void __launch_bounds__(256) buckets_renumber_kernel(uint32_t num_buckets, gp_voxel_bucket* __restrict__ buckets, const int* __restrict__ perm) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= num_buckets) return;
  const int v = buckets[b].voxel_index;
  if (v >= 0) buckets[b].voxel_index = perm[v];
}

// the binned build's statistics: the ordered segmented sum (gp_voxelmap_kernels.hpp), finalized
__global__ void __launch_bounds__(256) segmented_stats_kernel(const float* __restrict__ points, const float* __restrict__ covs, const float* __restrict__ intensities,
                                                              int num_voxels, const int* __restrict__ cell_start, const int* __restrict__ order, double inv_leaf, double leaf,
                                                              VoxelOutputs out, const gp::FillJob fill_buckets) {
  gp::run_fill_job(fill_buckets);  // (the bucket table the insertion kernel behind this one claims its slots in: 0xff = empty)
  SegmentSums sum;
  if (!segmented_sums(points, covs, intensities, num_voxels, cell_start, order, inv_leaf, leaf, sum)) return;
  emit_voxel(out, sum.v, sum.n, sum.acc, sum.imax, sum.cx, sum.cy, sum.cz, sum.ox, sum.oy, sum.oz);
}


// reference-visible bucket table from the list of DISTINCT voxels: claim the first free bucket of the probe chain
// (reference hash + max_bucket_scan_count rule, so lookup_voxel finds it); failed[0] += points of a voxel whose chain is full
__global__ void __launch_bounds__(256) insert_voxels_kernel(int num_voxels, const int* __restrict__ voxel_coords, const int* __restrict__ num_points,
                                                            gp_voxel_bucket* __restrict__ buckets, uint32_t num_buckets, uint32_t mask, int max_scan,
                                                            int* __restrict__ failed) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num_voxels) return;
  const int cx = voxel_coords[3 * (size_t)v], cy = voxel_coords[3 * (size_t)v + 1], cz = voxel_coords[3 * (size_t)v + 2];
  const uint64_t hash = coord_hash(cx, cy, cz);
  for (int j = 0; j < max_scan; j++) {
    gp_voxel_bucket* b = buckets + bucket_index(hash, j, num_buckets, mask);
    if (atomicCAS(&b->voxel_index, -1, v) == -1) {
      b->coord[0] = cx;
      b->coord[1] = cy;
      b->coord[2] = cz;
      return;
    }
  }
  *failed = 1;  // (a flag, not a count: the caller doubles the table until nothing fails; host-mapped on the binned build's path)
}
// lookup_voxels_kernel (cuda/kernels/lookup_voxels.cuh:34-60): voxel index of delta * p, or -1
__global__ void __launch_bounds__(256) lookup_kernel(const float* __restrict__ points, const float* __restrict__ normals, int n, VoxelMapView map,
                                                     const double* __restrict__ pose, int* __restrict__ out, int* __restrict__ hit_count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  int v = -1;
  if (i < n) {
    const Pose T = load_pose(pose);
    const double px = (double)points[3 * (size_t)i], py = (double)points[3 * (size_t)i + 1], pz = (double)points[3 * (size_t)i + 2];
    const double qx = T.r00 * px + T.r01 * py + T.r02 * pz + T.tx;
    const double qy = T.r10 * px + T.r11 * py + T.r12 * pz + T.ty;
    const double qz = T.r20 * px + T.r21 * py + T.r22 * pz + T.tz;
    bool rejected = !finite3(qx, qy, qz);  // a NaN / inf return lies in no voxel
    if (normals && !rejected) rejected = surface_rejected(T, qx, qy, qz, normals + 3 * (size_t)i);
    if (!rejected) v = lookup_voxel(map, fast_floor(qx * map.inv_leaf), fast_floor(qy * map.inv_leaf), fast_floor(qz * map.inv_leaf));
    if (out) out[i] = v;
  }
  if (hit_count) {
    const unsigned long long hits = __ballot(v >= 0);
    if ((threadIdx.x & 63) == 0 && hits) atomicAdd(hit_count, __popcll(hits));
  }
}

}  // namespace gp

gp::VoxelMapView gp_voxelmap::view() const {
  gp::VoxelMapView v;
  v.gblocks = has_grid ? gblocks.as<gp::GridBlock>() : nullptr;
  for (int a = 0; a < 3; a++) {
    v.glo[a] = grid.lo[a];
    v.gdim[a] = grid.dim[a];
  }
  v.plines = plines.as<gp_voxel_bucket>();
  v.plmask = plmask;
  v.pad_ = 0;
  v.buckets = buckets.as<gp_voxel_bucket>();
  v.records = records.as<gp::VoxelRecord>();
  v.voxel_coords = voxel_coords.as<int>();
  v.num_buckets = (uint32_t)info.num_buckets;
  v.bucket_mask = gp::pow2_mask(info.num_buckets);
  v.max_scan = info.max_bucket_scan_count;
  v.num_voxels = info.num_voxels;
  v.inv_leaf = 1.0 / resolution;
  v.leaf = resolution;
  return v;
}

namespace {

int bucket_limit_exceeded(const char* api) { return gp::fail(GP_ERROR_INVALID_ARGUMENT, std::string(api) + ": bucket table would exceed 2^30 entries"); }

// scratch of the hashed build's stages; it lives until the build returns (letting go of an array waits for the device)
struct HashedScratch {
  gp::DeviceArray rep, counters, sums;
};

}  // namespace

int gp::alloc_voxel_arrays(gp_voxelmap* m) {
  for (int id = gp_voxelmap::kRecords; id <= gp_voxelmap::kIntensities; id++) GP_TRY(m->arrays[id].dev.alloc_pooled(m->array_bytes(id), m->stream));
  return GP_OK;
}

// called at the end of a hashed insert, of an assign / reload without a grid, and by ensure_private_table
int gp::build_private_table(gp_voxelmap* m, hipStream_t s) {
  const int V = m->info.num_voxels;
  uint32_t lines = 256;
  while (lines < 2u * (uint32_t)std::max(V, 1)) lines <<= 1;  // 4 key slots per line: load factor <= 1/8
  m->plmask = lines - 1;
  GP_TRY(m->plines.alloc_pooled(64 * (size_t)lines, s));
  GP_HIP(hipMemsetAsync(m->plines.ptr, 0xff, 64 * (size_t)lines, s));
  if (V > 0) {
    hipLaunchKernelGGL(gp::line_claim_kernel, dim3(gp::blocks_of(V)), dim3(256), 0, s, V, m->voxel_coords.as<int>(), m->plines.as<gp_voxel_bucket>(), m->plmask);
    GP_HIP(hipGetLastError());
  }
  m->private_built = true;
  return GP_OK;
}

int gp_voxelmap::ensure_private_table() {
  std::lock_guard<std::mutex> lock(private_mutex);
  if (private_built) return GP_OK;
  if (!loaded()) return gp::fail(GP_ERROR_NOT_LOADED, "voxel map is not loaded on the GPU");
  GP_TRY(gp::build_private_table(this, stream));
  GP_HIP(hipStreamSynchronize(stream));
  return GP_OK;
}

// (kMaxGridBlocks, gp_binning.hpp: at most 2^24 blocks (256 MB) per map; a larger box keeps the hashed tables only)
bool gp::grid_geometry(const int bbox[6], gp::GridGeom* g, long long* num_blocks) {
  double nb = 1.0;
  for (int a = 0; a < 3; a++) {
    g->lo[a] = bbox[a];
    const long long d = (long long)bbox[3 + a] - (long long)bbox[a] + 1;
    if (d <= 0 || d > (1ll << 30)) return false;
    g->dim[a] = (int)d;
    nb *= (double)d;
  }
  if (nb > (double)gp::kMaxGridBlocks) return false;
  *num_blocks = (long long)g->dim[0] * g->dim[1] * g->dim[2];
  return true;
}

// box[] (in: the box so far, out: joined with the block-unit box of the set's living voxels), through the six device ints bbox_dev.  Synchronises the stream
int gp::voxels_bbox(const gp::VoxelSet& set, int* bbox_dev, int box[6], hipStream_t s) {
  GP_HIP(hipMemcpyAsync(bbox_dev, box, sizeof(int) * 6, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(gp::voxels_bbox_kernel, dim3(gp::blocks_of(set.num)), dim3(256), 0, s, set, bbox_dev);
  GP_HIP(hipGetLastError());
  GP_HIP(hipMemcpyAsync(box, bbox_dev, sizeof(int) * 6, hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));
  return GP_OK;
}

// the block grid of the sets' living voxels in blocks[nb]: zero -> bits -> counts -> exclusive scan of blocks[].base (scan_scratch: scan_scratch_ints(nb) ints; the
// scan leaves its grand total, the number of voxels, behind its block sums: gp_scan.hpp).  Asynchronous on `s`
int gp::build_block_grid(const gp::GridGeom& g, long long nb, gp::GridBlock* blocks, int* scan_scratch, const gp::VoxelSet* sets, int num_sets, hipStream_t s) {
  GP_HIP(hipMemsetAsync(blocks, 0, sizeof(gp::GridBlock) * (size_t)nb, s));
  for (int i = 0; i < num_sets; i++) {
    if (sets[i].num <= 0) continue;
    hipLaunchKernelGGL(gp::grid_mark_kernel, dim3(gp::blocks_of(sets[i].num)), dim3(256), 0, s, sets[i], g, blocks);
    GP_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(gp::grid_count_kernel, dim3(gp::blocks_of((size_t)nb)), dim3(256), 0, s, nb, blocks);
  GP_HIP(hipGetLastError());
  return gp::exclusive_scan_strided(&blocks[0].base, 4, &blocks[0].base, 4, nb, scan_scratch, s);
}

// device build of the occupancy-block grid: bounding box -> occupancy bits -> prefix sums -> voxels renumbered in
// (block, bit) order.  On return voxel_coords and the reference bucket table carry the NEW numbering (nothing else has been
// computed per voxel yet).  Synchronises the stream.
static int build_grid_device(gp_voxelmap* m, hipStream_t s) {
  m->has_grid = false;
  m->gblocks.release();
  const int V = m->info.num_voxels;
  if (V <= 0) return GP_OK;
  gp::DeviceArray d_bbox;
  GP_TRY(d_bbox.alloc(sizeof(int) * 6));
  int h_bbox[6];
  gp::empty_bbox(h_bbox);
  const gp::VoxelSet voxels{V, m->voxel_coords.as<int>(), nullptr, 0, 0, 0};
  GP_TRY(gp::voxels_bbox(voxels, d_bbox.as<int>(), h_bbox, s));
  gp::GridGeom g;
  long long nb = 0;
  if (!gp::grid_geometry(h_bbox, &g, &nb)) return GP_OK;
  gp::DeviceArray scratch, perm, coords_new;
  GP_TRY(m->gblocks.alloc(sizeof(gp::GridBlock) * (size_t)nb));
  GP_TRY(scratch.alloc(sizeof(int) * gp::scan_scratch_ints(nb)));
  GP_TRY(perm.alloc(sizeof(int) * (size_t)V));
  GP_TRY(coords_new.alloc(sizeof(int) * 3 * (size_t)V));
  gp::GridBlock* blocks = m->gblocks.as<gp::GridBlock>();
  GP_TRY(gp::build_block_grid(g, nb, blocks, scratch.as<int>(), &voxels, 1, s));
  hipLaunchKernelGGL(gp::grid_renumber_kernel, dim3(gp::blocks_of(V)), dim3(256), 0, s, V, m->voxel_coords.as<int>(), g, (const gp::GridBlock*)blocks, perm.as<int>(),
                     coords_new.as<int>());
  GP_HIP(hipGetLastError());
  hipLaunchKernelGGL(gp::buckets_renumber_kernel, dim3(gp::blocks_of((size_t)m->info.num_buckets)), dim3(256), 0, s, (uint32_t)m->info.num_buckets,
                     m->buckets.as<gp_voxel_bucket>(), (const int*)perm.as<int>());
  GP_HIP(hipGetLastError());
  GP_HIP(hipStreamSynchronize(s));  // perm / scratch die with this scope
  m->voxel_coords.swap(coords_new);
  m->grid = g;
  m->has_grid = true;
  return GP_OK;
}

// where a table of V voxels enters the doubling sequence init, 2 init, 4 init, ...: the first size that holds them at the load factor (GP_TUNE_BUCKET_LOAD)
int64_t gp::entry_bucket_count(int64_t init, int load_percent, int V) {
  int64_t num_buckets = init;
  while (num_buckets * (int64_t)load_percent < 100 * (int64_t)V) num_buckets *= 2;
  return num_buckets;
}

// the reference-visible bucket table of V distinct voxels in buckets[*num_buckets], doubled along the sequence until insert_voxels_kernel places every voxel; no
// voxel is ever dropped.  The first table is the caller's: filled with "empty" by the FillJob of the kernel that produced the voxels (first_table_prefilled), else
// here.  "A voxel found no bucket" is a host-mapped word the kernel stores to -- no fill, no copy kernel; a table that turns out too small is the rare path and
// starts over, after the stream has drained (the table let go of is the one the failed attempt wrote).  On GP_OK the build so far on `s` is complete
// (HostWords::finish: a flag kernel behind it, polled -- gp_host.hpp)
int gp::place_voxels(const char* api, const int* coords, const int* num_points, int V, gp::DeviceArray& buckets, int64_t* num_buckets, int max_scan,
                     bool first_table_prefilled, hipStream_t s) {
  gp::HostWords hw;
  GP_TRY(gp::HostWords::get(&hw));
  for (bool first = true;; *num_buckets *= 2, first = false) {
    if (!first) {
      if (*num_buckets > gp::kMaxBuckets) return bucket_limit_exceeded(api);
      GP_HIP(hipStreamSynchronize(s));
      GP_TRY(buckets.ensure_pooled(sizeof(gp_voxel_bucket) * (size_t)*num_buckets, s));
    }
    if (!first || !first_table_prefilled) GP_HIP(hipMemsetAsync(buckets.ptr, 0xff, sizeof(gp_voxel_bucket) * (size_t)*num_buckets, s));
    reinterpret_cast<volatile int*>(hw.host)[12] = 0;
    if (V > 0) {
      hipLaunchKernelGGL(gp::insert_voxels_kernel, dim3(gp::blocks_of((size_t)V)), dim3(256), 0, s, V, coords, num_points, buckets.as<gp_voxel_bucket>(),
                         (uint32_t)*num_buckets, gp::pow2_mask(*num_buckets), max_scan, hw.dev + 12);
      GP_HIP(hipGetLastError());
    }
    GP_TRY(hw.finish(s));  // :250
    if (reinterpret_cast<volatile int*>(hw.host)[12] == 0) return GP_OK;
  }
}

// the binned build (default): gp_binning.hpp gives the occupancy-block grid, the voxel numbering (block order) and the points
// sorted by voxel (stable); the statistics are an ordered segmented sum, the reference-visible bucket table is filled from the
// list of distinct voxels.  Deterministic: two builds of the same cloud give bit-identical maps.
static int insert_binned(gp_voxelmap* m, gp::PointBins& bins, const float* points_dev, const float* covs_dev, const float* intensities_dev, hipStream_t s) {
  const int V = bins.num_cells;
  m->info.num_voxels = V;
  GP_TRY(gp::alloc_voxel_arrays(m));
  GP_TRY(m->voxel_coords.alloc_pooled(sizeof(int) * 3 * (size_t)std::max(V, 1), s));
  // the bucket table of the first insertion attempt (below) is allocated here already: the statistics kernel fills it with "empty" on its way (gp_host.hpp, FillJob)
  // the doubling sequence is entered where the voxels fit at a load factor <= 1/3: at 1/2 .. 2/3 some probe chain among 10^5 voxels exceeds max_bucket_scan_count almost
  // surely, and the failed attempt (fill + insertion + a synchronisation) was 45 us of the 2 M-point build (profiles/r04_build_timeline.txt)
  // (GP_TUNE_BUCKET_LOAD, per map: 33 % by default = up to twice the entries of round 3's 1.5 V, 16 B each -- 4.2 MB instead of 2.1 MB for the 73.7 k voxels of the
  // bench map; info.num_buckets / memory_usage_gpu report it.  The reference's own sequence starts at init_num_buckets and doubles until the drop rate is met.)
  int64_t num_buckets = gp::entry_bucket_count(m->init_num_buckets, m->bucket_load_percent, V);
  if (num_buckets > gp::kMaxBuckets) return bucket_limit_exceeded("gp_voxelmap_insert");
  GP_TRY(m->buckets.ensure_pooled(sizeof(gp_voxel_bucket) * (size_t)num_buckets, s));
  static_assert(sizeof(gp_voxel_bucket) == 16, "FillJob granules");
  hipLaunchKernelGGL(gp::segmented_stats_kernel, dim3((V + 15) / 16), dim3(256), 0, s, points_dev, covs_dev, intensities_dev, V, (const int*)bins.cell_start.as<int>(),
                     (const int*)bins.order.as<int>(), 1.0 / m->resolution, m->resolution, gp::voxel_outputs(m->arrays),
                     gp::fill_job(m->buckets.ptr, sizeof(gp_voxel_bucket) * (size_t)num_buckets, 0xffffffffu));
  GP_HIP(hipGetLastError());
  // occupancy-block grid: taken over from the bins
  m->gblocks.swap(bins.blocks);
  m->grid = bins.geom;
  m->has_grid = true;
  // reference-visible bucket table (create_bucket_table, :253-307): the reference doubles the table until the fraction of points
  // whose probe chain is exhausted is <= target_points_drop_rate and then drops those points; here the table is doubled along the
  // same sequence until every voxel is placed, so no point is ever dropped (the CPU map, the parity target, drops none either)
  m->private_built = false;  // (the hashed kernel family's line table is built when a batch first asks for it: gp_voxelmap::ensure_private_table)
  m->plines.release();
  GP_TRY(gp::place_voxels("gp_voxelmap_insert", m->voxel_coords.as<int>(), m->num_points.as<int>(), V, m->buckets, &num_buckets, m->info.max_bucket_scan_count, true, s));
  m->info.num_buckets = (int)num_buckets;
  return GP_OK;
}

// ---- the hashed build: the reference's own scheme -- claim buckets with atomicCAS, allocate voxel ids, accumulate with atomics (not bit-reproducible) ----

// stage 1, create_bucket_table (:253-307): double the table until the drop rate is met, then number the voxels.  Leaves buckets, voxel_coords, info.num_buckets and
// info.num_voxels; waits for the stream once per attempt and once for the voxel count
static int hashed_bucket_table(gp_voxelmap* m, const float* points_dev, int n, hipStream_t s, HashedScratch& scratch) {
  const double inv_leaf = 1.0 / m->resolution;
  gp::DeviceArray &rep = scratch.rep, &counters = scratch.counters;
  GP_TRY(counters.alloc(sizeof(int) * 2));
  int h_counters[2] = {0, 0};
  // the reference starts at init_num_buckets and doubles (one full pass over the points per attempt); a table needs more slots
  // than voxels and a LiDAR map rarely has fewer voxels than points / 16, so the doubling sequence is entered further up when
  // the cloud is large (same sequence, fewer wasted passes: 5 -> 2 for the 2 M-point bench map)
  int64_t num_buckets = m->init_num_buckets;
  while (num_buckets < n / 16) num_buckets *= 2;
  for (;; num_buckets *= 2) {
    if (num_buckets > gp::kMaxBuckets) return bucket_limit_exceeded("gp_voxelmap_insert");
    GP_TRY(rep.ensure(sizeof(int) * (size_t)num_buckets));
    GP_HIP(hipMemsetAsync(rep.ptr, 0xff, sizeof(int) * (size_t)num_buckets, s));
    GP_HIP(hipMemsetAsync(counters.ptr, 0, sizeof(int) * 2, s));
    if (n > 0) {
      hipLaunchKernelGGL(gp::claim_buckets_kernel, dim3(gp::blocks_of(n)), dim3(256), 0, s, points_dev, n, rep.as<int>(), (uint32_t)num_buckets, gp::pow2_mask(num_buckets),
                         m->info.max_bucket_scan_count, inv_leaf, counters.as<int>(), counters.as<int>() + 1);
      GP_HIP(hipGetLastError());
    }
    GP_HIP(hipMemcpyAsync(h_counters, counters.ptr, sizeof(int) * 2, hipMemcpyDeviceToHost, s));
    GP_HIP(hipStreamSynchronize(s));
    // :288, over the VALID points (h_counters[0] = points in no voxel: NaN / inf / out of range -- neither failures nor members)
    if (h_counters[1] == 0 || (double)h_counters[1] / (double)std::max(n - h_counters[0], 1) <= m->target_points_drop_rate) break;
  }
  GP_HIP(hipMemsetAsync(counters.ptr, 0, sizeof(int), s));  // counters[0] becomes the voxel count
  m->info.num_buckets = (int)num_buckets;
  GP_TRY(m->buckets.alloc(sizeof(gp_voxel_bucket) * (size_t)num_buckets));
  // upper bound of the voxel count = number of claimed buckets <= min(n, num_buckets)
  const size_t max_voxels = (size_t)std::min<int64_t>(std::max(n, 1), num_buckets);
  GP_TRY(m->voxel_coords.alloc(sizeof(int) * 3 * max_voxels));
  hipLaunchKernelGGL(gp::assign_voxels_kernel, dim3(gp::blocks_of((size_t)num_buckets)), dim3(256), 0, s, points_dev, rep.as<int>(), (uint32_t)num_buckets,
                     inv_leaf, m->buckets.as<gp_voxel_bucket>(), m->voxel_coords.as<int>(), counters.as<int>());
  GP_HIP(hipGetLastError());
  GP_HIP(hipMemcpyAsync(h_counters, counters.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));
  m->info.num_voxels = h_counters[0];
  return GP_OK;
}

// stage 2, accumulate + finalize (:218-250): the statistics of info.num_voxels voxels, through the bucket table of stage 1.  Asynchronous on the stream
static int hashed_statistics(gp_voxelmap* m, const float* points_dev, const float* covs_dev, const float* intensities_dev, int n, hipStream_t s, HashedScratch& scratch) {
  const int V = m->info.num_voxels;
  GP_TRY(gp::alloc_voxel_arrays(m));
  gp::DeviceArray& sums = scratch.sums;
  GP_TRY(sums.alloc(sizeof(double) * 9 * (size_t)std::max(V, 1)));
  GP_HIP(hipMemsetAsync(sums.ptr, 0, sizeof(double) * 9 * (size_t)std::max(V, 1), s));
  GP_HIP(hipMemsetAsync(m->num_points.ptr, 0, sizeof(int) * (size_t)std::max(V, 1), s));
  GP_HIP(hipMemsetAsync(m->voxel_intensities.ptr, 0, sizeof(float) * (size_t)std::max(V, 1), s));
  if (n > 0 && V > 0) {
    hipLaunchKernelGGL(gp::accumulate_kernel, dim3(gp::blocks_of(n)), dim3(256), 0, s, points_dev, covs_dev, intensities_dev, n, m->view(), sums.as<double>(),
                       m->num_points.as<int>(), m->voxel_intensities.as<unsigned int>());
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(gp::finalize_kernel, dim3(gp::blocks_of(V)), dim3(256), 0, s, V, m->resolution, m->voxel_coords.as<int>(), sums.as<double>(),
                       m->num_points.as<int>(), gp::voxel_outputs(m->arrays));
    GP_HIP(hipGetLastError());
  }
  return GP_OK;
}

static int insert_hashed(gp_voxelmap* m, const float* points_dev, const float* covs_dev, const float* intensities_dev, int n, hipStream_t s) {
  HashedScratch scratch;
  GP_TRY(hashed_bucket_table(m, points_dev, n, s, scratch));
  GP_TRY(build_grid_device(m, s));  // occupancy-block grid + canonical voxel numbering (block order); the bucket table and voxel_coords follow it
  GP_TRY(hashed_statistics(m, points_dev, covs_dev, intensities_dev, n, s, scratch));
  GP_TRY(gp::build_private_table(m, s));
  GP_HIP(hipStreamSynchronize(s));  // :250
  return GP_OK;
}

extern "C" {

int gp_voxelmap_create(double resolution, int init_num_buckets, int max_bucket_scan_count, double target_points_drop_rate, gp_stream_t stream,
                       gp_voxelmap_t** out) {
  if (!out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_create: null out");
  if (!(resolution > 0.0) || init_num_buckets <= 0 || max_bucket_scan_count <= 0)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_create: resolution, init_num_buckets and max_bucket_scan_count must be positive");
  auto* m = new gp_voxelmap;
  m->resolution = resolution;
  m->init_num_buckets = init_num_buckets;
  m->target_points_drop_rate = target_points_drop_rate;
  m->stream = (hipStream_t)stream;
  m->info.num_voxels = 0;
  m->info.num_buckets = init_num_buckets;
  m->info.max_bucket_scan_count = max_bucket_scan_count;
  m->info.voxel_resolution = (float)resolution;
  *out = m;
  return GP_OK;
}

int gp_voxelmap_destroy(gp_voxelmap_t* map) {
  if (!map) return GP_OK;
  // the arrays go back to the device's memory pool: nothing may still be reading them (what hipFree would have waited for)
  (void)hipDeviceSynchronize();
  delete map;
  return GP_OK;
}

int gp_voxelmap_insert(gp_voxelmap_t* m, const float* points_dev, const float* covs_dev, const float* intensities_dev, int n) {
  if (!m) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_insert: null map");
  if (!points_dev || !covs_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "error: GPU points/covs not allocated!!");  // gaussian_voxelmap_gpu.cu:212-215
  if (n < 0) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_insert: negative size");
  hipStream_t s = m->stream;
  // re-inserting into a map that already holds arrays releases them to the block cache ("any stream may take them"): kernels of other streams
  // that still read the old map must have finished.  A fresh map has nothing to wait for.
  if (m->buckets.ptr) GP_HIP(hipDeviceSynchronize());
  m->drop_incremental_state();  // (an incremental map is replaced like any other, and counts its inserts from zero again)
  m->offloaded = false;
  m->generation++;
  if (n > 0 && !m->force_hashed_build) {
    gp::PointBins bins;
    bool too_large = false;
    GP_TRY(gp::bin_points(points_dev, n, 1.0 / m->resolution, s, &bins, &too_large));
    if (!too_large && bins.num_cells > 0) return insert_binned(m, bins, points_dev, covs_dev, intensities_dev, s);
  }
  // an empty cloud, a cloud whose bounding box is too large for the block grid, or GP_TUNE_MAP_BUILD
  return insert_hashed(m, points_dev, covs_dev, intensities_dev, n, s);
}

int gp_voxelmap_info_get(const gp_voxelmap_t* map, gp_voxelmap_info* info) {
  if (!map || !info) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_info_get: null");
  *info = map->info;
  return GP_OK;
}

double gp_voxelmap_resolution(const gp_voxelmap_t* map) { return map ? map->resolution : 0.0; }

int gp_voxelmap_views_get(const gp_voxelmap_t* map, gp_voxelmap_views* views) {
  if (!map || !views) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_views_get: null");
  const bool on = map->loaded();
  views->buckets = on ? map->buckets.as<gp_voxel_bucket>() : nullptr;
  views->num_points = on ? map->num_points.as<int>() : nullptr;
  views->voxel_means = on ? map->voxel_means.as<float>() : nullptr;
  views->voxel_covs = on ? map->voxel_covs.as<float>() : nullptr;
  views->voxel_intensities = on ? map->voxel_intensities.as<float>() : nullptr;
  return GP_OK;
}

int gp_voxelmap_loaded_on_gpu(const gp_voxelmap_t* map) { return map && map->loaded() ? 1 : 0; }
int gp_voxelmap_has_block_grid(const gp_voxelmap_t* map) { return map && map->has_grid ? 1 : 0; }
// per map: GP_TUNE_MAP_BUILD = 1 builds with the reference-shaped hashed scheme (the fallback of clouds too large for the block grid; A/B and tests)
int gp_voxelmap_set_tuning(gp_voxelmap_t* map, int key, int value) {
  if (!map) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_set_tuning: null map");
  if (key == GP_TUNE_BUCKET_LOAD) {
    if (value < 5 || value > 90) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_set_tuning: GP_TUNE_BUCKET_LOAD is a load factor in per cent, 5 .. 90");
    map->bucket_load_percent = value;
    return GP_OK;
  }
  if (key != GP_TUNE_MAP_BUILD) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_set_tuning: the keys of a voxel map are GP_TUNE_MAP_BUILD and GP_TUNE_BUCKET_LOAD");
  map->force_hashed_build = value != 0;
  return GP_OK;
}

int gp_voxelmap_lookup(const gp_voxelmap_t* map, const float* points_dev, const float* normals_dev, int n, const double delta[16], int* voxel_indices_dev,
                       gp_stream_t stream) {
  // (an empty cloud has no arrays: n == 0 asks for no pointer)
  if (!map || !delta || n < 0 || (n > 0 && (!points_dev || !voxel_indices_dev))) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_lookup: bad arguments");
  if (!map->loaded()) return gp::fail(GP_ERROR_NOT_LOADED, "gp_voxelmap_lookup: voxel map is not on the GPU");
  if (n == 0) return GP_OK;
  hipStream_t s = (hipStream_t)stream;
  gp::DeviceArray pose;
  GP_TRY(pose.alloc(sizeof(double) * 16));
  GP_HIP(hipMemcpyAsync(pose.ptr, delta, sizeof(double) * 16, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(gp::lookup_kernel, dim3(gp::blocks_of(n)), dim3(256), 0, s, points_dev, normals_dev, n, map->view(), pose.as<double>(), voxel_indices_dev,
                     (int*)nullptr);
  GP_HIP(hipGetLastError());
  GP_HIP(hipStreamSynchronize(s));
  return GP_OK;
}

int gp_voxelmap_overlap(const gp_voxelmap_t* map, const float* points_dev, int n, const double delta[16], int* num_hits, gp_stream_t stream) {
  if (!map || !delta || !num_hits || n < 0 || (n > 0 && !points_dev)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_overlap: bad arguments");
  if (!map->loaded()) return gp::fail(GP_ERROR_NOT_LOADED, "gp_voxelmap_overlap: voxel map is not on the GPU");
  *num_hits = 0;
  if (n == 0) return GP_OK;
  hipStream_t s = (hipStream_t)stream;
  gp::DeviceArray scratch;
  GP_TRY(scratch.alloc(sizeof(double) * 16 + sizeof(int) * 4));
  int* d_count = reinterpret_cast<int*>(scratch.as<double>() + 16);
  GP_HIP(hipMemcpyAsync(scratch.ptr, delta, sizeof(double) * 16, hipMemcpyHostToDevice, s));
  GP_HIP(hipMemsetAsync(d_count, 0, sizeof(int), s));
  hipLaunchKernelGGL(gp::lookup_kernel, dim3(gp::blocks_of(n)), dim3(256), 0, s, points_dev, (const float*)nullptr, n, map->view(), scratch.as<double>(),
                     (int*)nullptr, d_count);
  GP_HIP(hipGetLastError());
  GP_HIP(hipMemcpyAsync(num_hits, d_count, sizeof(int), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));
  return GP_OK;
}

}  // extern "C"
