// gp_voxelmap_store.hip -- where a built voxel map goes and comes from: download to the host, assign from host arrays (with the host build of the block grid),
// save_compact / load, clone to another device, memory usage, offload / reload.  Nothing here depends on which build made the map (the binned build is the default:
// gp_voxelmap.hip), and no kernel is launched from here except the line table's, through gp::build_private_table.
// Offload, reload, clone and the downloads walk the one table of the map's arrays (gp_voxelmap::arrays, gp_host.hpp).
//
// Replaces src/gtsam_points/types/gaussian_voxelmap_gpu.cu: save/load :309-467, offload/reload :469-535, download_* :537-571.
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>

#include "gp_voxelmap.hpp"

namespace {

// GaussianVoxelData (types/gaussian_voxel_data.hpp:11-54): 56-byte on-disk record
struct VoxelDataRecord {
  int coord[3];
  int num_points;
  float mean[3];
  float cov[6];  // xx xy xz yy yz zz
  float intensity;
};
static_assert(sizeof(VoxelDataRecord) == 56, "GaussianVoxelData must be 56 B");

// host build of the block grid, the structure of build_grid_device (gp_voxelmap.hip), for assign: returns the permutation old index -> new index
bool build_grid_host(int V, const int* coords, gp::GridGeom* g, std::vector<gp::GridBlock>* blocks, std::vector<int>* perm) {
  if (V <= 0) return false;
  int bbox[6];
  gp::empty_bbox(bbox);
  for (int v = 0; v < V; v++)
    for (int a = 0; a < 3; a++) {
      bbox[a] = std::min(bbox[a], coords[3 * (size_t)v + a] >> 2);
      bbox[3 + a] = std::max(bbox[3 + a], coords[3 * (size_t)v + a] >> 2);
    }
  long long nb = 0;
  if (!gp::grid_geometry(bbox, g, &nb)) return false;
  blocks->assign((size_t)nb, gp::GridBlock{0ull, 0, 0});
  for (int v = 0; v < V; v++) {
    const int* c = coords + 3 * (size_t)v;
    (*blocks)[(size_t)gp::grid_block_index(*g, c[0], c[1], c[2])].bits |= 1ull << gp::grid_bit(c[0], c[1], c[2]);
  }
  int run = 0;
  for (auto& b : *blocks) {
    b.base = run;
    run += __builtin_popcountll(b.bits);
  }
  if (run != V) return false;  // duplicate coordinates in the input: no canonical numbering
  perm->resize((size_t)V);
  for (int v = 0; v < V; v++) {
    const int* c = coords + 3 * (size_t)v;
    const gp::GridBlock& b = (*blocks)[(size_t)gp::grid_block_index(*g, c[0], c[1], c[2])];
    (*perm)[(size_t)v] = b.base + __builtin_popcountll(b.bits & ((1ull << gp::grid_bit(c[0], c[1], c[2])) - 1ull));
  }
  return true;
}

// array `id` of the map to `dst`, or nothing when the caller does not ask for it or the array is empty.  Asynchronous on the map's stream
int fetch(const gp_voxelmap* m, int id, void* dst) {
  if (dst && m->array_bytes(id)) GP_HIP(hipMemcpyAsync(dst, m->arrays[id].dev.ptr, m->array_bytes(id), hipMemcpyDeviceToHost, m->stream));
  return GP_OK;
}

}  // namespace

extern "C" {

int gp_voxelmap_download(const gp_voxelmap_t* map, gp_voxel_bucket* buckets, int* num_points, float* means, float* covs, float* intensities) {
  if (!map) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_download: null map");
  if (!map->loaded()) return gp::fail(GP_ERROR_NOT_LOADED, "gp_voxelmap_download: voxel map is not on the GPU");
  GP_TRY(fetch(map, gp_voxelmap::kBuckets, buckets));
  GP_TRY(fetch(map, gp_voxelmap::kNumPoints, num_points));
  GP_TRY(fetch(map, gp_voxelmap::kMeans, means));
  GP_TRY(fetch(map, gp_voxelmap::kCovs, covs));
  GP_TRY(fetch(map, gp_voxelmap::kIntensities, intensities));
  GP_HIP(hipStreamSynchronize(map->stream));
  return GP_OK;
}

int gp_voxelmap_download_f64(const gp_voxelmap_t* map, int* coords, int* num_points, double* means, double* covs) {
  if (!map) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_download_f64: null map");
  if (!map->loaded()) return gp::fail(GP_ERROR_NOT_LOADED, "gp_voxelmap_download_f64: voxel map is not on the GPU");
  const size_t V = (size_t)map->info.num_voxels;
  if (V == 0) return GP_OK;
  std::vector<gp::VoxelRecord> recs(V);
  std::vector<int> h_coords(3 * V);
  GP_TRY(fetch(map, gp_voxelmap::kRecords, recs.data()));
  GP_TRY(fetch(map, gp_voxelmap::kCoords, h_coords.data()));
  GP_HIP(hipStreamSynchronize(map->stream));
  for (size_t v = 0; v < V; v++) {
    if (coords) memcpy(coords + 3 * v, h_coords.data() + 3 * v, sizeof(int) * 3);
    if (num_points) num_points[v] = recs[v].num_points;
    if (means)
      for (int k = 0; k < 3; k++) means[3 * v + k] = ((double)h_coords[3 * v + k] + 0.5) * map->resolution + (double)recs[v].mean_local[k];
    if (covs) gp::sym6_to_full(recs[v].cov, covs + 9 * v);
  }
  return GP_OK;
}

// host half of GaussianVoxelMapGPU::load (gaussian_voxelmap_gpu.cu:413-466): probe limit = max_bucket_scan_count,
// table starts at 8192*4 buckets and doubles until every voxel fits
int gp_voxelmap_assign(gp_voxelmap_t* m, int num_voxels, const int* coords, const int* num_points, const float* means, const float* covs6,
                       const float* intensities) {
  if (!m || num_voxels < 0) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_assign: bad arguments");
  if (num_voxels > 0 && (!coords || !num_points || !means || !covs6)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_assign: null arrays");
  const size_t V = (size_t)num_voxels;
  // occupancy-block grid + canonical (block-order) numbering: the input arrays are permuted before anything is derived from them
  gp::GridGeom geom{};
  std::vector<gp::GridBlock> h_blocks;
  std::vector<int> perm, p_coords, p_np;
  std::vector<float> p_means, p_covs6, p_int;
  const bool grid = build_grid_host(num_voxels, coords, &geom, &h_blocks, &perm);
  if (grid) {
    p_coords.resize(3 * V);
    p_np.resize(V);
    p_means.resize(3 * V);
    p_covs6.resize(6 * V);
    if (intensities) p_int.resize(V);
    for (size_t v = 0; v < V; v++) {
      const size_t nv = (size_t)perm[v];
      memcpy(p_coords.data() + 3 * nv, coords + 3 * v, sizeof(int) * 3);
      p_np[nv] = num_points[v];
      memcpy(p_means.data() + 3 * nv, means + 3 * v, sizeof(float) * 3);
      memcpy(p_covs6.data() + 6 * nv, covs6 + 6 * v, sizeof(float) * 6);
      if (intensities) p_int[nv] = intensities[v];
    }
    coords = p_coords.data();
    num_points = p_np.data();
    means = p_means.data();
    covs6 = p_covs6.data();
    if (intensities) intensities = p_int.data();
  }
  std::vector<gp_voxel_bucket> h_buckets;
  const int max_scan = m->info.max_bucket_scan_count;
  auto assign_buckets = [&](int64_t nb) {
    h_buckets.assign((size_t)nb, gp_voxel_bucket{{0, 0, 0}, -1});
    const uint32_t mask = gp::pow2_mask(nb);
    for (size_t i = 0; i < V; i++) {
      const uint64_t hash = gp::coord_hash(coords[3 * i], coords[3 * i + 1], coords[3 * i + 2]);
      bool inserted = false;
      for (int j = 0; j < max_scan; j++) {
        auto& b = h_buckets[gp::bucket_index(hash, j, (uint32_t)nb, mask)];
        if (b.voxel_index < 0) {
          b.coord[0] = coords[3 * i];
          b.coord[1] = coords[3 * i + 1];
          b.coord[2] = coords[3 * i + 2];
          b.voxel_index = (int)i;
          inserted = true;
          break;
        }
      }
      if (!inserted) return false;
    }
    return true;
  };
  int64_t nb = 8192 * 4;
  for (; nb < gp::kMaxBuckets; nb *= 2)
    if (assign_buckets(nb)) break;
  if (nb >= gp::kMaxBuckets) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_assign: could not build the bucket table");

  std::vector<gp::VoxelRecord> recs(V);
  std::vector<float> h_covs(9 * V), h_int(V, 0.0f);
  for (size_t v = 0; v < V; v++) {
    for (int k = 0; k < 3; k++) {
      const double centre = ((double)coords[3 * v + k] + 0.5) * m->resolution;
      recs[v].mean_local[k] = (float)((double)means[3 * v + k] - centre);
    }
    recs[v].num_points = num_points[v];
    for (int k = 0; k < 6; k++) recs[v].cov[k] = (double)covs6[6 * v + k];
    gp::sym6_to_full(covs6 + 6 * v, h_covs.data() + 9 * v);
    if (intensities) h_int[v] = intensities[v];
  }
  if (m->has_sums) {  // (an incremental map is replaced like any other: gp_voxelmap_insert)
    GP_HIP(hipDeviceSynchronize());
    m->drop_incremental_state();
  }
  m->info.num_voxels = num_voxels;
  m->info.num_buckets = (int)nb;
  m->offloaded = false;
  m->generation++;
  hipStream_t s = m->stream;
  GP_TRY(m->buckets.alloc(sizeof(gp_voxel_bucket) * (size_t)nb));
  GP_TRY(gp::alloc_voxel_arrays(m));
  GP_TRY(m->voxel_coords.alloc(sizeof(int) * 3 * std::max<size_t>(V, 1)));
  GP_HIP(hipMemcpyAsync(m->buckets.ptr, h_buckets.data(), sizeof(gp_voxel_bucket) * (size_t)nb, hipMemcpyHostToDevice, s));
  if (V) {
    GP_HIP(hipMemcpyAsync(m->records.ptr, recs.data(), sizeof(gp::VoxelRecord) * V, hipMemcpyHostToDevice, s));
    GP_HIP(hipMemcpyAsync(m->num_points.ptr, num_points, sizeof(int) * V, hipMemcpyHostToDevice, s));
    GP_HIP(hipMemcpyAsync(m->voxel_means.ptr, means, sizeof(float) * 3 * V, hipMemcpyHostToDevice, s));
    GP_HIP(hipMemcpyAsync(m->voxel_covs.ptr, h_covs.data(), sizeof(float) * 9 * V, hipMemcpyHostToDevice, s));
    GP_HIP(hipMemcpyAsync(m->voxel_intensities.ptr, h_int.data(), sizeof(float) * V, hipMemcpyHostToDevice, s));
    GP_HIP(hipMemcpyAsync(m->voxel_coords.ptr, coords, sizeof(int) * 3 * V, hipMemcpyHostToDevice, s));
  }
  m->has_grid = false;
  m->gblocks.release();
  if (grid) {
    GP_TRY(m->gblocks.alloc(sizeof(gp::GridBlock) * h_blocks.size()));
    GP_HIP(hipMemcpyAsync(m->gblocks.ptr, h_blocks.data(), sizeof(gp::GridBlock) * h_blocks.size(), hipMemcpyHostToDevice, s));
    m->grid = geom;
    m->has_grid = true;
  }
  GP_HIP(hipStreamSynchronize(s));  // the staging vectors die with this scope
  m->private_built = false;
  if (!m->has_grid) {
    GP_TRY(gp::build_private_table(m, s));
    GP_HIP(hipStreamSynchronize(s));
  }
  return GP_OK;
}

int gp_voxelmap_save_compact(const gp_voxelmap_t* map, const char* path) {
  if (!map || !path) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_save_compact: null");
  if (!map->loaded()) return gp::fail(GP_ERROR_NOT_LOADED, "gp_voxelmap_save_compact: voxel map is not on the GPU");
  const size_t V = (size_t)map->info.num_voxels;
  std::vector<int> h_coords(3 * V), h_np(V);
  std::vector<float> h_means(3 * V), h_covs(9 * V), h_int(V);
  if (V) {
    GP_TRY(fetch(map, gp_voxelmap::kCoords, h_coords.data()));
    GP_TRY(gp_voxelmap_download(map, nullptr, h_np.data(), h_means.data(), h_covs.data(), h_int.data()));
  }
  std::vector<VoxelDataRecord> serial(V);
  for (size_t v = 0; v < V; v++) {
    auto& r = serial[v];
    memcpy(r.coord, h_coords.data() + 3 * v, sizeof(int) * 3);
    r.num_points = h_np[v];
    memcpy(r.mean, h_means.data() + 3 * v, sizeof(float) * 3);
    gp::full_to_sym6(h_covs.data() + 9 * v, r.cov);
    r.intensity = h_int[v];
  }
  std::ofstream ofs(path, std::ios::binary);
  if (!ofs) return gp::fail(GP_ERROR_IO, std::string("error: failed to open ") + path);
  // header of gaussian_voxelmap_gpu.cu:358-366
  ofs << "compact " << 1 << std::endl;
  {  // every digit of the double: load rebuilds mean_local and every later floor(p / resolution) from this value (the stream's default is 6 significant digits)
    std::ostringstream res;
    res.precision(std::numeric_limits<double>::max_digits10);
    res << map->resolution;
    ofs << "resolution " << res.str() << std::endl;
  }
  ofs << "lru_count " << 0 << std::endl;
  ofs << "lru_cycle " << 1 << std::endl;
  ofs << "lru_thresh " << 1 << std::endl;
  ofs << "voxel_bytes " << sizeof(VoxelDataRecord) << std::endl;
  ofs << "num_voxels " << serial.size() << std::endl;
  ofs.write(reinterpret_cast<const char*>(serial.data()), (std::streamsize)(sizeof(VoxelDataRecord) * serial.size()));
  return ofs ? GP_OK : gp::fail(GP_ERROR_IO, std::string("error: failed to write ") + path);
}

int gp_voxelmap_load(const char* path, gp_stream_t stream, gp_voxelmap_t** out) {
  if (!path || !out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_load: null");
  std::ifstream ifs(path, std::ios::binary);
  if (!ifs) return gp::fail(GP_ERROR_IO, std::string("error: failed to open ") + path);
  std::string token;
  bool compact = false;
  double resolution = 0.0;
  int lru = 0, voxel_bytes = 0, num_voxels = 0;
  ifs >> token >> compact;
  ifs >> token >> resolution;
  ifs >> token >> lru;
  ifs >> token >> lru;
  ifs >> token >> lru;
  ifs >> token >> voxel_bytes;
  ifs >> token >> num_voxels;
  std::getline(ifs, token);
  if (!ifs || voxel_bytes != (int)sizeof(VoxelDataRecord) || num_voxels < 0) return gp::fail(GP_ERROR_IO, std::string("error: malformed voxel map file ") + path);
  std::vector<VoxelDataRecord> flat((size_t)num_voxels);
  ifs.read(reinterpret_cast<char*>(flat.data()), (std::streamsize)(sizeof(VoxelDataRecord) * flat.size()));
  if (!ifs && num_voxels > 0) return gp::fail(GP_ERROR_IO, std::string("error: truncated voxel map file ") + path);
  const size_t V = flat.size();
  std::vector<int> coords(3 * V), np(V);
  std::vector<float> means(3 * V), covs6(6 * V), ints(V);
  for (size_t v = 0; v < V; v++) {  // (the record holds the six entries assign takes: no unpacking here)
    memcpy(coords.data() + 3 * v, flat[v].coord, sizeof(int) * 3);
    np[v] = flat[v].num_points;
    memcpy(means.data() + 3 * v, flat[v].mean, sizeof(float) * 3);
    memcpy(covs6.data() + 6 * v, flat[v].cov, sizeof(float) * 6);
    ints[v] = flat[v].intensity;
  }
  gp_voxelmap_t* m = nullptr;
  GP_TRY(gp_voxelmap_create(resolution, 8192, 10, 0.1, stream, &m));  // :451
  int rc = gp_voxelmap_assign(m, num_voxels, coords.data(), np.data(), means.data(), covs6.data(), ints.data());
  if (rc != GP_OK) {
    gp_voxelmap_destroy(m);
    return rc;
  }
  *out = m;
  return GP_OK;
}

// replica of a map on another device (multi-GPU sharding: a target map referenced from several shards).  Arrays travel
// device-to-device with hipMemcpyPeerAsync; the clone owns its memory and carries the same voxel numbering.
int gp_voxelmap_clone_to_device(const gp_voxelmap_t* map, int device, gp_stream_t stream_on_device, gp_voxelmap_t** out) {
  if (!map || !out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_clone_to_device: null");
  if (!map->loaded()) return gp::fail(GP_ERROR_NOT_LOADED, "gp_voxelmap_clone_to_device: voxel map is not on the GPU");
  int src_device = 0, saved = 0;
  GP_HIP(hipGetDevice(&saved));
  {
    hipPointerAttribute_t attr{};
    src_device = (hipPointerGetAttributes(&attr, map->buckets.ptr) == hipSuccess) ? attr.device : saved;
    (void)hipGetLastError();
  }
  GP_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream_on_device;
  auto* m = new gp_voxelmap;
  m->resolution = map->resolution;
  m->init_num_buckets = map->init_num_buckets;
  m->target_points_drop_rate = map->target_points_drop_rate;
  m->stream = s;
  m->info = map->info;
  m->plmask = map->plmask;
  m->has_grid = map->has_grid;
  m->grid = map->grid;
  m->has_sums = map->has_sums;
  m->lru_counter = map->lru_counter;
  m->lru_horizon = map->lru_horizon;
  m->lru_clear_cycle = map->lru_clear_cycle;
  int rc = GP_OK;
  auto copy = [&](gp::DeviceArray& dst, const gp::DeviceArray& src, size_t bytes) {
    if (rc != GP_OK) return;
    if ((rc = dst.alloc(bytes)) != GP_OK) return;
    if (bytes == 0) return;
    const hipError_t e = hipMemcpyPeerAsync(dst.ptr, device, src.ptr, src_device, bytes, s);
    if (e != hipSuccess) rc = gp::hip_fail(e, "hipMemcpyPeerAsync", __FILE__, __LINE__);
  };
  for (int id = 0; id < gp_voxelmap::kGblocks; id++) copy(m->arrays[id].dev, map->arrays[id].dev, map->array_bytes(id));
  if (map->private_built) copy(m->plines, map->plines, 64 * ((size_t)map->plmask + 1));
  m->private_built = map->private_built;
  if (map->has_grid) copy(m->gblocks, map->gblocks, map->array_bytes(gp_voxelmap::kGblocks));
  if (rc == GP_OK) {
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = gp::hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
  }
  (void)hipSetDevice(saved);
  if (rc != GP_OK) {
    delete m;
    return rc;
  }
  m->generation = 1;
  *out = m;
  return GP_OK;
}

size_t gp_voxelmap_memory_usage_gpu(const gp_voxelmap_t* map) {
  if (!map) return 0;
  // reference formula (gaussian_voxelmap_gpu.cu:469-472) + the gather records, coordinates and line table this implementation adds (not a sum over the table of
  // arrays: like the reference's, it leaves the intensities out)
  // (an incremental map's sums and stamps: their rows of the table)
  return map->array_bytes(gp_voxelmap::kSums) + map->array_bytes(gp_voxelmap::kStamps) +
         (size_t)map->info.num_voxels * (sizeof(int) + sizeof(float) * 3 + sizeof(float) * 9 + sizeof(gp::VoxelRecord) + sizeof(int) * 3) +
         (size_t)map->info.num_buckets * sizeof(gp_voxel_bucket) + (map->private_built ? ((size_t)map->plmask + 1) * 4 * sizeof(gp_voxel_bucket) : 0) +
         (map->has_grid ? (size_t)map->num_grid_blocks() * sizeof(gp::GridBlock) : 0);
}

int gp_voxelmap_offload(gp_voxelmap_t* m, gp_stream_t stream) {
  if (!m) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_offload: null");
  if (!m->loaded()) return GP_ERROR_NOT_LOADED;  // reference returns false (:477-479)
  hipStream_t s = (hipStream_t)stream;
  for (int id = 0; id < gp_voxelmap::kNumArrays; id++) {  // (a map without a grid keeps an empty copy of gblocks)
    auto& a = m->arrays[id];
    a.host.resize(m->array_bytes(id));
    if (!a.host.empty()) GP_HIP(hipMemcpyAsync(a.host.data(), a.dev.ptr, a.host.size(), hipMemcpyDeviceToHost, s));
  }
  // the arrays go back to the per-thread block cache tagged "any stream may take them": a factor kernel on ANOTHER stream may still be reading
  // the map (the caller offloads while a linearise is in flight on the factor's stream), so every stream of the device is drained first -- what
  // hipFree used to imply; an offload is a rare, millisecond-scale operation
  GP_HIP(hipDeviceSynchronize());
  for (int id = 0; id < gp_voxelmap::kGblocks; id++) m->arrays[id].dev.release();
  m->plines.release();
  m->private_built = false;
  m->gblocks.release();
  m->offloaded = true;
  m->generation++;
  return GP_OK;
}

int gp_voxelmap_reload(gp_voxelmap_t* m, gp_stream_t stream) {
  if (!m) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_reload: null");
  if (!m->offloaded) return GP_ERROR_INVALID_ARGUMENT;  // already on the GPU: reference returns false (:509-511)
  hipStream_t s = (hipStream_t)stream;
  const int num = m->has_grid ? gp_voxelmap::kNumArrays : gp_voxelmap::kGblocks;  // (gblocks, the last of the table: only when there is a grid)
  for (int id = 0; id < num; id++) {
    auto& a = m->arrays[id];
    GP_TRY(a.dev.alloc(a.host.size()));
    if (!a.host.empty()) GP_HIP(hipMemcpyAsync(a.dev.ptr, a.host.data(), a.host.size(), hipMemcpyHostToDevice, s));
  }
  m->private_built = false;
  if (!m->has_grid) GP_TRY(gp::build_private_table(m, s));  // (with a grid the line table waits for its first use: gp_voxelmap::ensure_private_table)
  GP_HIP(hipStreamSynchronize(s));
  m->offloaded = false;
  m->generation++;
  return GP_OK;
}

}  // extern "C"
