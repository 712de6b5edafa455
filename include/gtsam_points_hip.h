/*
 * gtsam_points_hip.h -- C-ABI of libgtsam_points_hip.so
 *
 * MI355X (gfx950) native replacement for the CUDA half of koide3/gtsam_points' VGICP
 * path.  This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Every entry point cites the reference interface it replaces (paths relative to the
 * reference tree, v1.2.1).  The reference-side binding a maintainer would add is shown
 * in INTEGRATION.md; gtsam_points_amd/host/ holds a C++ mirror of the reference classes
 * written against this header.
 *
 * Conventions
 *   - All functions return 0 (GP_OK) on success, non-zero otherwise; gp_last_error()
 *     returns a thread-local message.  (The reference logs CUDA errors to stderr and
 *     continues, cuda/check_error.cu:8-18; the C++ mirror reproduces that on top of the
 *     status codes.)
 *   - Matrices are COLUMN-MAJOR (Eigen default).  A pose is double[16], the 4x4
 *     T_target^-1 * T_source ("delta") -- the double-precision analogue of the
 *     Eigen::Isometry3f the reference uploads (integrated_vgicp_factor_gpu.cpp:136-164).
 *     Double is required for <=1e-5 parity with the CPU IntegratedVGICPFactor.
 *   - Source clouds are caller-owned device arrays in the reference's GPU layout
 *     (types/point_cloud.hpp:114-118): points float[N][3], covs float[N][9] (column-major
 *     3x3), normals float[N][3] (optional).  The library never frees them.
 *   - Covariances: all nine entries are read.  A symmetric matrix (what estimate_covariances
 *     produces after the cast to float) is used as it is; of a non-symmetric one the kernels use
 *     the symmetric part (a_ij + a_ji) / 2, formed in double -- the part the reference CPU
 *     factor's full 3x3 algebra sees to first order in the asymmetry (the HessianFactor keeps
 *     only the upper triangle of H, integrated_matching_cost_factor.cpp:49).
 *   - gp_stream_t is a hipStream_t (the reference's CUstream_st*).  NULL = default stream.
 *   - Handles are thread-compatible (external synchronisation per handle).
 *   - Ownership: handles hold raw pointers, not references.  A factor points at its voxel map and its source arrays, a batch /
 *     multi-batch / factor set at its factors: destroy in the order batch -> factor -> map, and keep the source arrays alive as
 *     long as a factor uses them (the reference holds shared_ptrs; the C++ mirror does the same on top of these handles).
 *     gp_vgicp_factor_destroy / gp_vgicp_batch_destroy do not synchronise a caller-owned stream (the reference's clone() drops it
 *     first): finish the work on it before destroying.
 */
#ifndef GTSAM_POINTS_HIP_H
#define GTSAM_POINTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GP_OK 0
#define GP_ERROR_INVALID_ARGUMENT 1
#define GP_ERROR_HIP 2
#define GP_ERROR_NOT_LOADED 3 /* voxel map / cloud offloaded from the GPU */
#define GP_ERROR_IO 4
#define GP_ERROR_INDETERMINATE 5 /* normal equations not positive definite (IndeterminantLinearSystemException upstream) */
/* The rule of every damped step (dense and sparse, one launch or several): the Cholesky factorisation calls the system indeterminate when a pivot p is not above
 * 1e-11 x the damped assembled diagonal entry of its column (A_pp + the damping + the prior, before any elimination).  A pivot is the entry after the elimination of
 * the columns in front of it, so the rule reads: min_p pivot_p / A~_pp <= 1e-11 -> GP_ERROR_INDETERMINATE. */

typedef void* gp_stream_t; /* hipStream_t */

/* ---- runtime (replaces cuda/check_error, cuda/cuda_stream, cuda/cuda_memory, cuda_device_*) ---- */

const char* gp_last_error(void);
const char* gp_version(void);
int gp_device_count(int* count);                                /* cuda/cuda_device_names */
int gp_set_device(int device);
int gp_get_device(int* device);
int gp_device_name(int device, char* name, size_t name_len);    /* cuda_device_names() */
int gp_device_synchronize(void);                                /* cuda/cuda_device_sync.cu */
/* Scratch and structure arrays are stream-ordered pool blocks; released ones are parked in a bounded per-thread cache (<= 96 blocks,
 * <= 4 GiB) and re-used by the next build on the same stream.  This returns the calling thread's parked blocks to the pool, and releases the (up to four) side
 * streams + events gp_estimate_covariances keeps per host thread and device: a long-lived pool thread that is done with a device calls it once. */
int gp_trim_device_cache(void);
int gp_stream_create(gp_stream_t* stream);                      /* cuda/cuda_stream.cu (cudaStreamNonBlocking) */
int gp_stream_destroy(gp_stream_t stream);
int gp_stream_synchronize(gp_stream_t stream);
int gp_malloc(void** ptr, size_t bytes);                        /* cuda/cuda_malloc_async.hpp */
int gp_free(void* ptr);
int gp_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, gp_stream_t stream); /* async; caller syncs */
int gp_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, gp_stream_t stream); /* async; caller syncs */
int gp_memcpy_d2d(void* dst_dev, const void* src_dev, size_t bytes, gp_stream_t stream);  /* async; caller syncs */
int gp_memset(void* dst_dev, int value, size_t bytes, gp_stream_t stream);
int gp_host_malloc(void** ptr, size_t bytes);                   /* pinned staging, cuda/cuda_buffer.cu */
int gp_host_free(void* ptr);

/* ---- StreamRoundRobin / TempBufferManager / StreamTempBufferRoundRobin ----
 * cuda/stream_roundrobin.hpp:14-31, cuda/stream_temp_buffer_roundrobin.hpp:19-65 */

typedef struct gp_temp_buffer gp_temp_buffer_t;
typedef struct gp_stream_pool gp_stream_pool_t;

int gp_temp_buffer_create(size_t init_buffer_size, gp_temp_buffer_t** out);  /* TempBufferManager(size) */
int gp_temp_buffer_get(gp_temp_buffer_t* tb, size_t size, void** dev_ptr);   /* get_buffer(): grow-only, x1.2 */
int gp_temp_buffer_clear(gp_temp_buffer_t* tb);                              /* keep the newest buffer */
int gp_temp_buffer_clear_all(gp_temp_buffer_t* tb);
int gp_temp_buffer_destroy(gp_temp_buffer_t* tb);

int gp_stream_pool_create(int num_streams, size_t init_buffer_size, gp_stream_pool_t** out); /* defaults 4, 512 KiB */
int gp_stream_pool_get(gp_stream_pool_t* pool, gp_stream_t* stream, gp_temp_buffer_t** buffer); /* get_stream_buffer() */
int gp_stream_pool_sync_all(gp_stream_pool_t* pool);
int gp_stream_pool_clear(gp_stream_pool_t* pool);
int gp_stream_pool_clear_all(gp_stream_pool_t* pool);
int gp_stream_pool_destroy(gp_stream_pool_t* pool);

/* ---- GaussianVoxelMapGPU : types/gaussian_voxelmap_gpu.hpp:20-114, .cu:25-573 ---- */

/* VoxelMapInfo, gaussian_voxelmap_gpu.hpp:20-25 */
typedef struct gp_voxelmap_info {
  int num_voxels;
  int num_buckets;
  int max_bucket_scan_count;
  float voxel_resolution;
} gp_voxelmap_info;

/* VoxelBucket {Eigen::Vector3i first; int second}, gaussian_voxelmap_gpu.hpp:30-33 (16 B) */
typedef struct gp_voxel_bucket {
  int coord[3];
  int voxel_index; /* < 0 : empty */
} gp_voxel_bucket;

/* raw device views = the reference's public data members (gaussian_voxelmap_gpu.hpp:86-101) */
typedef struct gp_voxelmap_views {
  const gp_voxel_bucket* buckets; /* [num_buckets] */
  const int* num_points;          /* [num_voxels] */
  const float* voxel_means;       /* [num_voxels][3] */
  const float* voxel_covs;        /* [num_voxels][9] column-major */
  const float* voxel_intensities; /* [num_voxels] */
} gp_voxelmap_views;

typedef struct gp_voxelmap gp_voxelmap_t;

/* GaussianVoxelMapGPU(resolution, init_num_buckets=16384, max_bucket_scan_count=10,
 *                     target_points_drop_rate=1e-3, stream), gaussian_voxelmap_gpu.cu:176-198.
 * resolution is double so that voxel coordinates are computed exactly as the CPU map does
 * (fast_floor(x * (1.0/leaf)), gaussian_voxelmap_cpu.cpp:59-61).
 * Deviation: the default (binned) build keeps EVERY voxel -- like the CPU map -- and sizes the reference-visible bucket table by
 * doubling from init_num_buckets until every voxel is inserted within max_bucket_scan_count probes (the sequence is entered at the first size >= 3 x the
 * number of voxels: a fuller table almost surely fails an attempt); target_points_drop_rate is
 * honoured only by the reference-shaped hashed build (gp_voxelmap_set_tuning(GP_TUNE_MAP_BUILD, 1) and the fallback for huge bounding boxes), whose
 * doubling sequence starts at the first size >= N/16, so with a drop rate > 0 num_buckets and the set of dropped points can
 * differ from the reference's. */
int gp_voxelmap_create(double resolution, int init_num_buckets, int max_bucket_scan_count, double target_points_drop_rate, gp_stream_t stream, gp_voxelmap_t** out);
int gp_voxelmap_destroy(gp_voxelmap_t* map);
/* insert(const PointCloud&): one-shot build from device arrays, gaussian_voxelmap_gpu.cu:211-307.
 * intensities_dev may be NULL (voxel intensities = 0, :232-240).  Returns when everything it issued on the map's stream has finished (a polled completion
 * flag behind the last kernel; a stream synchronisation when that takes longer than 0.5 ms).  The hashed kernel family's private line table is built on first use. */
int gp_voxelmap_insert(gp_voxelmap_t* map, const float* points_dev, const float* covs_dev, const float* intensities_dev, int num_points);
/* The INCREMENTAL insert with LRU eviction -- GaussianVoxelMapCPU::insert (gaussian_voxelmap_cpu.cpp:23-47), i.e. IncrementalVoxelMap<GaussianVoxel>::insert
 * (ann/impl/incremental_voxelmap_impl.hpp:31-68); the reference's GPU map has none.  The frame's points are ADDED to the voxels the map holds (count, f64 sums,
 * max intensity), the voxels it touches are stamped with the map's counter, the counter is incremented, and on every lru_clear_cycle-th call the voxels with
 * stamp + lru_horizon < counter are dropped (with lru_horizon = 0 the ones just touched too); means and covariances are the sums over the counts.  An empty frame
 * (num_points == 0: the arrays may be NULL) still counts and may evict.  Non-finite and out-of-range points are skipped as by gp_voxelmap_insert.
 * The map starts empty (or as an incremental map): one that holds voxels built by gp_voxelmap_insert / _assign / _load is refused (GP_ERROR_INVALID_ARGUMENT), and so
 * is a frame with which the map's box would exceed the block grid (2^24 blocks of 4x4x4 voxels) -- the map, its counter and its generation are unchanged then.
 * gp_voxelmap_insert on an incremental map replaces it as on any other and resets the counter.  Deterministic: two maps fed the same frames hold the same bits.
 * Factors built on the map notice the new contents through its generation, like after gp_voxelmap_insert. */
int gp_voxelmap_insert_incremental(gp_voxelmap_t* map, const float* points_dev, const float* covs_dev, const float* intensities_dev, int num_points);
/* lru_horizon >= 0 and lru_clear_cycle >= 1 (defaults 10 / 10, ann/incremental_voxelmap.hpp); the counter, the horizon and the cycle (any pointer may be NULL) */
int gp_voxelmap_set_lru(gp_voxelmap_t* map, int64_t lru_horizon, int64_t lru_clear_cycle);
int gp_voxelmap_lru_get(const gp_voxelmap_t* map, int64_t* lru_counter, int64_t* lru_horizon, int64_t* lru_clear_cycle);
/* int64 out_host[num_voxels]: the counter value of the insert that last touched each voxel.  Refused for a map with voxels that took no incremental insert. */
int gp_voxelmap_download_stamps(const gp_voxelmap_t* map, int64_t* out_host);
int gp_voxelmap_info_get(const gp_voxelmap_t* map, gp_voxelmap_info* info);
double gp_voxelmap_resolution(const gp_voxelmap_t* map);                       /* voxel_resolution() */
int gp_voxelmap_views_get(const gp_voxelmap_t* map, gp_voxelmap_views* views);
/* download_buckets / download_voxel_num_points / _means / _covs / _intensities, gaussian_voxelmap_gpu.cu:537-571.
 * Host buffers sized from gp_voxelmap_info. Any pointer may be NULL. Synchronous. */
int gp_voxelmap_download(const gp_voxelmap_t* map, gp_voxel_bucket* buckets, int* num_points, float* means, float* covs, float* intensities);
/* full-precision voxel statistics (double means[V][3], covs[V][9] col-major) for parity tests */
int gp_voxelmap_download_f64(const gp_voxelmap_t* map, int* coords, int* num_points, double* means, double* covs);
/* rebuild from flat voxel records (the host half of GaussianVoxelMapGPU::load, gaussian_voxelmap_gpu.cu:372-467):
 * coords int[V][3], num_points int[V], means float[V][3], covs6 float[V][6] (xx,xy,xz,yy,yz,zz), intensities float[V] */
int gp_voxelmap_assign(gp_voxelmap_t* map, int num_voxels, const int* coords, const int* num_points, const float* means, const float* covs6, const float* intensities);
/* save_compact(path) / load(path): text header + GaussianVoxelData records, types/gaussian_voxel_data.hpp:11-54,
 * gaussian_voxelmap_gpu.cu:309-370, :372-467; interoperable with GaussianVoxelMapCPU::save_compact/load. */
int gp_voxelmap_save_compact(const gp_voxelmap_t* map, const char* path);
int gp_voxelmap_load(const char* path, gp_stream_t stream, gp_voxelmap_t** out);
/* OffloadableGPU: memory_usage_gpu / loaded_on_gpu / offload_gpu / reload_gpu, gaussian_voxelmap_gpu.cu:469-535 */
size_t gp_voxelmap_memory_usage_gpu(const gp_voxelmap_t* map);
int gp_voxelmap_loaded_on_gpu(const gp_voxelmap_t* map);
/* 1 when the map carries the occupancy-block grid the default VGICP kernel looks voxels up in (bounding box <= 2^24 blocks of
 * 4x4x4 voxels), 0 when only the hashed tables exist (the kernels then use those) */
int gp_voxelmap_has_block_grid(const gp_voxelmap_t* map);
int gp_voxelmap_offload(gp_voxelmap_t* map, gp_stream_t stream);
int gp_voxelmap_reload(gp_voxelmap_t* map, gp_stream_t stream);
/* correspondence lookup of delta * p for every source point -> voxel index or -1
 * (lookup_voxels_kernel, cuda/kernels/lookup_voxels.cuh:19-97); normals_dev!=NULL enables surface validation */
int gp_voxelmap_lookup(const gp_voxelmap_t* map, const float* points_dev, const float* normals_dev, int num_points, const double delta[16], int* voxel_indices_dev, gp_stream_t stream);
/* overlap_gpu(target, source, delta): number of source points that hit a voxel,
 * types/gaussian_voxelmap_gpu_funcs.cu:192-236.  Synchronous. */
int gp_voxelmap_overlap(const gp_voxelmap_t* map, const float* points_dev, int num_points, const double delta[16], int* num_hits, gp_stream_t stream);
/* overlap_gpu(targets, source, Ts_target_source): number of source points that fall in a voxel of ANY target
 * (deltas = [num_targets][16] column-major doubles), types/gaussian_voxelmap_gpu_funcs.cu:265-335.  Synchronous. */
int gp_voxelmap_overlap_multi(const gp_voxelmap_t* const* targets, const double* deltas, int num_targets, const float* points_dev, int num_points, int* num_hits,
                              gp_stream_t stream);
/* overlap_gpu(targets, sources, Ts_target_source) -> one count per (target[i], source[i]) pair, one launch for all pairs,
 * types/gaussian_voxelmap_gpu_funcs.cu:337-404.  Synchronous. */
int gp_voxelmap_overlap_batch(const gp_voxelmap_t* const* targets, const float* const* points_dev, const int* num_points, const double* deltas, int num_pairs,
                              int* num_hits, gp_stream_t stream);

/* ---- merge_frames_gpu : types/gaussian_voxelmap_gpu_funcs.cu:65-152 ----
 * gp_transform_frames: out[begin_i + j] = pose_i * frame_i[j] for all frames in one launch (transform_means_kernel /
 * transform_covs_kernel, :42-62; f64 arithmetic on the f32 inputs).  out_covs_dev / out_intensities_dev may be NULL;
 * a NULL intensities entry yields zeros (:103-107).  Synchronous.
 * gp_merge_frames: the transform followed by the Gaussian voxel-map build at downsample_resolution (:122-123, the
 * reference hard-codes init_num_buckets = total points, scan count 10, drop rate 1e-3); the merged cloud is the returned
 * map's voxel_means / voxel_covs / voxel_intensities views (caller owns the map). */
int gp_transform_frames(const double* poses, const float* const* points_dev, const float* const* covs_dev, const float* const* intensities_dev, const int* num_points,
                        int num_frames, float* out_points_dev, float* out_covs_dev, float* out_intensities_dev, gp_stream_t stream);
int gp_merge_frames(const double* poses, const float* const* points_dev, const float* const* covs_dev, const float* const* intensities_dev, const int* num_points,
                    int num_frames, double downsample_resolution, double target_points_drop_rate, gp_stream_t stream, gp_voxelmap_t** out_map);

/* ---- PointCloudGPU::add_points_gpu / add_normals_gpu / add_covs_gpu : types/point_cloud_gpu.cu:26-62,110-201 ----
 * src_host: num_points vectors (vec3) or column-major matrices (mat3) of dimension src_dim in {3,4}, double or float,
 * exactly as the reference's Eigen::Matrix<T, D, 1> / <T, D, D> arrays lie in memory; dst_dev: float[N][3] / float[N][9].
 * The conversion runs on the device (the reference converts element-wise on the host).  Synchronous. */
int gp_cloud_upload_vec3(const void* src_host, int src_is_double, int src_dim, int num_points, float* dst_dev, gp_stream_t stream);
int gp_cloud_upload_mat3(const void* src_host, int src_is_double, int src_dim, int num_points, float* dst_dev, gp_stream_t stream);

/* ---- LinearizedSystem6 : cuda/kernels/linearized_system.cuh:10-71 ----
 * Same fields, double precision, no Eigen alignment padding; num_inliers is carried as a double so
 * that a stack of records is a homogeneous f64 array (sum-reducible with one RCCL all-reduce).
 * HessianFactor convention (applied by the caller): (H_target, H_target_source, -b_target, H_source, -b_source, error),
 * integrated_vgicp_factor_gpu.cpp:199-213. */
typedef struct gp_linearized6 {
  double num_inliers;
  double error;
  double H_target[36];
  double H_source[36];
  double H_target_source[36];
  double b_target[6];
  double b_source[6];
} gp_linearized6; /* 122 doubles = 976 B */

/* the reference's own float record layout (496 B with Eigen's 16-B alignment), for callers that kept it */
typedef struct gp_linearized6_f32 {
  int num_inliers;
  float error;
  float pad_[2];
  float H_target[36];
  float H_source[36];
  float H_target_source[36];
  float b_target[6];
  float b_source[6];
} gp_linearized6_f32;
void gp_linearized6_to_f32(const gp_linearized6* in, gp_linearized6_f32* out);

/* ---- IntegratedVGICPDerivatives / IntegratedVGICPFactorGPU device half ----
 * factors/integrated_vgicp_derivatives.cuh, integrated_vgicp_derivatives*.cu,
 * factors/integrated_vgicp_factor_gpu.cpp:136-272 */

typedef struct gp_vgicp_factor gp_vgicp_factor_t;

/* IntegratedVGICPDerivatives(target, source, stream, temp_buffer), integrated_vgicp_derivatives.cu:19-47.
 * Borrows the map handle and the three device arrays (normals_dev may be NULL).  stream==NULL -> the factor
 * creates and owns a non-blocking stream (:36-39); temp_buffer==NULL -> it owns its scratch (:41-43).
 * Source points with a NaN / inf coordinate have no correspondence (they count neither as inliers nor towards H, b, the error). */
int gp_vgicp_factor_create(const gp_voxelmap_t* target, const float* points_dev, const float* covs_dev, const float* normals_dev, int num_points, gp_stream_t stream, gp_temp_buffer_t* temp_buffer, gp_vgicp_factor_t** out);
int gp_vgicp_factor_destroy(gp_vgicp_factor_t* f);
int gp_vgicp_factor_set_surface_validation(gp_vgicp_factor_t* f, int enable); /* set_enable_surface_validation */
/* the source cloud's device arrays moved (PointCloudGPU::offload_gpu + reload_gpu, types/point_cloud_gpu.cu:304-370):
 * hand the factor the new pointers; every batch holding the factor rebuilds its table on the next issue */
int gp_vgicp_factor_set_source(gp_vgicp_factor_t* f, const float* points_dev, const float* covs_dev, const float* normals_dev);
/* Packed source mirrors.  The stream kernels read a private 36-B-per-point repack of (points_dev, covs_dev) -- replaces the per-point reads of
 * include/gtsam_points/cuda/kernels/vgicp_derivatives.cuh:36-50 -- built once per cloud at a factor's first table build and shared by every factor
 * on the same (points_dev, covs_dev, num_points).  The borrowed arrays are therefore IMMUTABLE while a factor holds them (the reference holds them through
 * PointCloud::ConstPtr).  An owner that rewrites them in place, or frees them while the address may be handed out again, calls
 * gp_source_mirror_invalidate(ptr) (forget mirrors built from ptr, so that later factors pack afresh) and gp_vgicp_factor_set_source on the factors
 * that keep using the cloud (same or new pointers: the factor drops its mirror and packs again).  gp_source_mirror_bytes: device bytes of all live mirrors. */
int gp_source_mirror_invalidate(const void* dev_ptr);
int64_t gp_source_mirror_bytes(void);
int gp_vgicp_factor_set_inlier_update_thresh(gp_vgicp_factor_t* f, double trans, double angle); /* kept for API parity; every linearise rescans all points */
int gp_vgicp_factor_num_points(const gp_vgicp_factor_t* f);
int gp_vgicp_factor_device(const gp_vgicp_factor_t* f); /* the device the source arrays live on */
gp_stream_t gp_vgicp_factor_stream(const gp_vgicp_factor_t* f);
/* sizes the factor reports through NonlinearFactorGPU (integrated_vgicp_factor_gpu.cpp:136-150):
 * 128 (pose, double[16]) / 976 (gp_linearized6) / 128 / 8 (double error) */
size_t gp_vgicp_linearization_input_size(void);
size_t gp_vgicp_linearization_output_size(void);
size_t gp_vgicp_evaluation_input_size(void);
size_t gp_vgicp_evaluation_output_size(void);
/* issue_linearize(lin_input_cpu, lin_input_gpu, lin_output_gpu), integrated_vgicp_factor_gpu.cpp:229-237 +
 * integrated_vgicp_derivatives_linearize.cu:23-55.  Asynchronous on the factor's stream.  pose_dev is the device
 * copy of the pose (double[16]); out_dev receives one gp_linearized6.  No alignment beyond 8 B is assumed. */
int gp_vgicp_factor_issue_linearize(gp_vgicp_factor_t* f, const double* pose_host, const double* pose_dev, gp_linearized6* out_dev);
/* issue_compute_error(lin cpu, eval cpu, lin gpu, eval gpu, out gpu), integrated_vgicp_factor_gpu.cpp:247-263 +
 * integrated_vgicp_derivatives_compute.cu:23-39: correspondences and fused covariance at pose_lin, residual at pose_eval. */
int gp_vgicp_factor_issue_compute_error(gp_vgicp_factor_t* f, const double* pose_lin_host, const double* pose_eval_host, const double* pose_lin_dev, const double* pose_eval_dev, double* out_dev);
int gp_vgicp_factor_sync(gp_vgicp_factor_t* f);                               /* sync_stream() */
/* synchronous fall-backs (IntegratedVGICPDerivatives::linearize / compute_error, integrated_vgicp_derivatives.cu:80-109) */
int gp_vgicp_factor_linearize(gp_vgicp_factor_t* f, const double pose[16], gp_linearized6* out_host);
int gp_vgicp_factor_compute_error(gp_vgicp_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host);

/* ---- NonlinearFactorSetGPU fast path: one batched launch over a factor table ----
 * replaces the per-factor loop of cuda/nonlinear_factor_set_gpu.cpp:64-218 (F x {reduce, select} launches,
 * 2F stream syncs) by ONE tiled launch over all factors' points for a synchronous rigid-pose call (poses read where the caller left them, the workgroup that
 * stores a factor's last partial row finalizes the factor, records and completion words go straight into host-mapped memory), and by a tiled launch + a finalize
 * launch for the asynchronous entry points (device-resident records). */

typedef struct gp_vgicp_batch gp_vgicp_batch_t;

int gp_vgicp_batch_create(gp_vgicp_factor_t* const* factors, int num_factors, gp_stream_t stream, gp_vgicp_batch_t** out);
int gp_vgicp_batch_destroy(gp_vgicp_batch_t* batch);
int gp_vgicp_batch_size(const gp_vgicp_batch_t* batch);
int64_t gp_vgicp_batch_total_points(const gp_vgicp_batch_t* batch);
int64_t gp_vgicp_batch_algorithmic_bytes(const gp_vgicp_batch_t* batch); /* sum 48 N + 16 buckets + 52 voxels + 560 */
/* what a pass of the batch's built table really requests with perfect reuse of the lookup structures: the source stream as the kernel reads it (36 B per point
 * through the packed mirrors, GP_TUNE_SOURCE_MIRROR, else 48; + 12 with surface validation), each distinct map's block grid (or bucket table) and 64-B records once,
 * pose in, record out.  Reported beside the algorithmic figure, which internal repacking does not change. */
int64_t gp_vgicp_batch_actual_bytes(gp_vgicp_batch_t* batch);
/* asynchronous on the batch stream; poses_host = double[F][16]; out_dev = gp_linearized6[F] in device memory */
int gp_vgicp_batch_issue_linearize(gp_vgicp_batch_t* batch, const double* poses_host, gp_linearized6* out_dev);
int gp_vgicp_batch_issue_compute_error(gp_vgicp_batch_t* batch, const double* poses_lin_host, const double* poses_eval_host, double* out_dev);
int gp_vgicp_batch_sync(gp_vgicp_batch_t* batch);
/* the two asynchronous passes with the pose tables ALREADY in device memory (double[F][16] each, column-major: what the device-side retract of gp_lm_graph_* produces):
 * nothing is staged or copied, the host has nothing to wait for.  Same kernels, same records.  rigid != 0: the caller vouches that every 3x3 block is orthonormal to
 * 1e-9 -- the test the host-pose entry points make themselves to choose between the 29-sum kernel + adjoint expansion and the 92-sum kernel that is exact for any block */
int gp_vgicp_batch_issue_linearize_dev(gp_vgicp_batch_t* batch, const double* poses_dev, int rigid, gp_linearized6* out_dev);
/* Which kernels the host-pose entry points run at these poses (double[F][16] / double[16], column-major): *out = 1, the 29 sums + adjoint expansion -- every 3x3
 * block orthonormal to 1e-9 and no pose FAR, i.e. |t| <= GP_TUNE_FAR_POSE_RATIO x the largest |coordinate| of the factor's source cloud; *out = 0, the explicit-J_s
 * sums (all f64, from the source point itself).  The expansion H_s = Ad^T H_t Ad cancels about (|t| / |p|)^2 of the f32 rounding in H_t, so a scan registered against
 * a map whose origin is kilometres away takes the explicit sums.  One far or non-orthonormal pose decides for the whole batch.  Pass the answer as `rigid` to
 * gp_vgicp_batch_issue_linearize_dev to get what the host-pose entry points would run (gp_lm_graph_set_values does). */
int gp_vgicp_batch_takes_rigid_path(gp_vgicp_batch_t* batch, const double* poses_host, int* out);
int gp_vgicp_factor_takes_rigid_path(gp_vgicp_factor_t* factor, const double pose[16], int* out);
int gp_vgicp_batch_issue_compute_error_dev(gp_vgicp_batch_t* batch, const double* poses_lin_dev, const double* poses_eval_dev, double* out_dev);
/* ... and the error evaluation as a synchronous call that POLLS the finalize kernel's completion words (pinned) instead of synchronising the stream: on return everything
 * queued in front of it on the batch's stream is complete, work queued behind it meanwhile is not waited for.  _begin / _end: the same in two halves (one begin at a time). */
int gp_vgicp_batch_compute_error_dev(gp_vgicp_batch_t* batch, const double* poses_lin_dev, const double* poses_eval_dev, double* out_host);
int gp_vgicp_batch_issue_compute_error_dev_begin(gp_vgicp_batch_t* batch, const double* poses_lin_dev, const double* poses_eval_dev);
int gp_vgicp_batch_compute_error_dev_end(gp_vgicp_batch_t* batch, double* out_host);
int gp_vgicp_batch_stream(const gp_vgicp_batch_t* batch, gp_stream_t* out); /* the stream the batch was created on */
/* synchronous: upload poses, compute, download F records into out_host */
int gp_vgicp_batch_linearize(gp_vgicp_batch_t* batch, const double* poses_host, gp_linearized6* out_host);
/* the same pass without the copy into a caller array: *out_view points at the F records where the kernels stored them (the
 * batch's pinned, host-mapped result buffer), valid until the next call on this batch.  The 976 bytes per factor are then read once,
 * by their consumer (NonlinearFactorSetGPU's store_linearized loop), instead of copied first: 6 us of a 98 us 256-factor pass,
 * 12 us of a 289 us 512-factor pass (profiles/r02_sync_batch_overheads.txt) */
int gp_vgicp_batch_linearize_view(gp_vgicp_batch_t* batch, const double* poses_host, const gp_linearized6** out_view);
int gp_vgicp_batch_compute_error(gp_vgicp_batch_t* batch, const double* poses_lin_host, const double* poses_eval_host, double* out_host);
/* timing hook for bench.py: re-runs only the device work (pose upload excluded) `iters` times on the batch stream
 * between two hipEvents and returns the average milliseconds per pass, and separately the two kernels' times */
int gp_vgicp_batch_time_linearize(gp_vgicp_batch_t* batch, const double* poses_host, int iters, float* ms_total, float* ms_main_kernel, float* ms_finalize_kernel);

/* ---- many-factor batches sharded over the GPUs of one node, driven from ONE process ----
 * The reference has no multi-GPU code; this is the sharded form of NonlinearFactorSetGPU::linearize
 * (cuda/nonlinear_factor_set_gpu.cpp:64-139) that BASELINE.json's north_star asks for: the factor list is partitioned into
 * shards, every shard runs the batched kernels on its own device and stream, every shard writes its records into its rows of a
 * zeroed [F x 122] f64 stack, ONE ncclAllReduce(sum) per device over that stack (RCCL over xGMI; each row has one writer, so the
 * sum is exact), one D2H from the first shard's device.  RCCL is dlopen()ed only when a multi-batch spans several devices. */

/* contiguous partition of a factor list into num_shards ranges minimising the largest sum of weights (weights = source points of
 * each factor; list the factors source-submap-major so that a shard holds whole submaps).  Pure host code: needs no GPU. */
typedef struct gp_shard_plan gp_shard_plan_t;
int gp_shard_plan_create(const int64_t* weights, int num_factors, int num_shards, gp_shard_plan_t** out);
int gp_shard_plan_num_shards(const gp_shard_plan_t* plan);
int gp_shard_plan_range(const gp_shard_plan_t* plan, int shard, int* begin, int* end); /* factors [begin, end) */
int gp_shard_plan_destroy(gp_shard_plan_t* plan);

/* a voxel map replicated onto another device (maps are immutable after insert(): a shard that references a target map of a
 * neighbouring shard gets its own copy; arrays travel device-to-device).  The clone is independent of the original. */
int gp_voxelmap_clone_to_device(const gp_voxelmap_t* map, int device, gp_stream_t stream_on_device, gp_voxelmap_t** out);

typedef struct gp_vgicp_multi_batch gp_vgicp_multi_batch_t;
/* factors[i] must have been created from arrays / a map resident on the device of its shard.
 * shard_of_factor == NULL: one shard per device the factors live on (num_shards ignored).  Otherwise shard_of_factor[i] in
 * [0, num_shards): several shards may share a device (the single-GPU rehearsal of an N-GPU plan).
 * use_rccl: 0 = no collective: every shard's finalize kernel stores its records straight into its rows of one host-pinned, portable stack; 1 = ncclAllReduce(sum)
 * of the zeroed [F x 122] f64 stack (required: error when the shards share a device or librccl.so does not load; one shard on one device is a valid 1-rank
 * communicator); 2 = in-place ncclAllGather when the shards are equal contiguous ranges in rank order (what gp_shard_plan deals for equal weights: half the bytes of
 * the all-reduce, no zeroing), else the all-reduce; -1 = automatic: 2 when the shards sit on distinct devices and librccl.so loads, else 0.
 * gp_vgicp_multi_batch_uses_rccl: 0 no collective, 1 all-reduce, 2 all-gather. */
int gp_vgicp_multi_batch_create(gp_vgicp_factor_t* const* factors, int num_factors, const int* shard_of_factor, int num_shards, int use_rccl,
                                gp_vgicp_multi_batch_t** out);
int gp_vgicp_multi_batch_destroy(gp_vgicp_multi_batch_t* mb);
int gp_vgicp_multi_batch_size(const gp_vgicp_multi_batch_t* mb);
int gp_vgicp_multi_batch_num_shards(const gp_vgicp_multi_batch_t* mb);
int gp_vgicp_multi_batch_uses_rccl(const gp_vgicp_multi_batch_t* mb);
int gp_vgicp_multi_batch_shard_info(const gp_vgicp_multi_batch_t* mb, int shard, int* device, int* num_factors, int64_t* num_points);
/* synchronous; poses_host = double[F][16] and out_host = gp_linearized6[F] in the order of `factors` */
int gp_vgicp_multi_batch_linearize(gp_vgicp_multi_batch_t* mb, const double* poses_host, gp_linearized6* out_host);
int gp_vgicp_multi_batch_compute_error(gp_vgicp_multi_batch_t* mb, const double* poses_lin_host, const double* poses_eval_host, double* out_host);
/* HIP-event times of the last pass: the slowest shard's kernels, and what followed them (all-reduce + D2H, or the host gather) */
int gp_vgicp_multi_batch_last_timing(const gp_vgicp_multi_batch_t* mb, float* ms_compute, float* ms_exchange);

/* ---- the exchange of the one-process-per-GPU form as direct stores over xGMI (gp_peer.hip; no reference counterpart: the reference has no multi-GPU code) ----
 * Every rank needs every rank's records (north_star: "all-reduce of the stacked H blocks").  For small exchanges -- the headline's 8 x 976 B -- a collective library is all
 * latency; here every rank stores its rows straight into a buffer of every peer (mapped through hipIpc handles the caller exchanges once), flags its arrival, waits for the
 * peers' flags and hands the complete [world][row_doubles] stack to the host: one single-workgroup kernel per step and rank.  row_doubles <= 8192, world <= 16.
 *   create   allocates this rank's buffer on the current device and writes its IPC handle (gp_peer_exchange_handle_bytes() bytes) to handle_out
 *   connect  handles = [world][handle bytes] in rank order (the own entry is ignored): maps the peers' buffers
 *   rows     this rank's [world][row_doubles] f64 stack of generation 0 / 1 on the device (two generations alternate; a rank's own rows go to row `rank`)
 *   begin    names the generation (0 / 1) whose stack the NEXT exchange fills; does not advance the step (a caller whose own kernels fail between begin and finish
 *            leaves the exchange where it was)
 *   finish   behind the kernels that wrote the rank's rows, on the same stream: the exchange kernel; host_out_pinned (may be NULL) = pinned [world][row_doubles] f64
 *            (checked: pageable or device memory is GP_ERROR_INVALID_ARGUMENT).  The step's sequence number advances here, once the kernel is launched
 *   check    after the stream's synchronisation: GP_OK, or an error when a peer did not arrive within the kernel's time box.  A rank that gives up poisons its
 *            arrival words at every peer, so all ranks fail in the same step; the exchange is then broken for good (destroy it, fall back to a collective)
 *   set_timeout_ms   the time box a rank waits for its peers (default 2000 ms; a rank skew above it -- a debugger, a long GC pause -- is an error here where a
 *            collective would wait) */
typedef struct gp_peer_exchange gp_peer_exchange_t;
int gp_peer_exchange_handle_bytes(void);
int gp_peer_exchange_create(int world, int rank, int row_doubles, gp_peer_exchange_t** out, void* handle_out);
int gp_peer_exchange_connect(gp_peer_exchange_t* px, const void* handles);
void* gp_peer_exchange_rows(gp_peer_exchange_t* px, int generation);
int gp_peer_exchange_begin(gp_peer_exchange_t* px);
int gp_peer_exchange_set_timeout_ms(gp_peer_exchange_t* px, double ms);
int gp_peer_exchange_finish(gp_peer_exchange_t* px, gp_stream_t stream, double* host_out_pinned);
int gp_peer_exchange_check(const gp_peer_exchange_t* px);
int gp_peer_exchange_destroy(gp_peer_exchange_t* px);

/* ---- exact k-NN, covariance estimation, GICP (BASELINE configs[4]; CPU-only upstream) ----
 * KdTree::knn_search (ann/small_kdtree.hpp:437-474, KnnResult ann/knn_result.hpp:36-117), estimate_covariances
 * (features/covariance_estimation.cpp:18-77), IntegratedGICPFactor (factors/impl/integrated_gicp_factor_impl.hpp:132-296) */

typedef struct gp_point_grid gp_point_grid_t; /* cell-sorted copy of a cloud: the GPU stand-in for the reference's KdTree */
int gp_point_grid_create(const float* points_dev, int num_points, double cell_size, gp_stream_t stream, gp_point_grid_t** out);
/* as above with a GP_TUNE_KNN_STRUCTURE value for THIS structure and, for measurement, a device buffer of 8 uint64 work counters the searches on it
 * add to (or NULL): {shell walks, f32 distance evaluations, f64 distance evaluations, block entries read, occupied cells visited, octant stages} */
int gp_point_grid_create_ex(const float* points_dev, int num_points, double cell_size, int structure, unsigned long long* counters_dev, gp_stream_t stream,
                            gp_point_grid_t** out);
int gp_point_grid_destroy(gp_point_grid_t* grid);
/* exact k nearest neighbours (1 <= k <= 32) of each query within max_sq_dist (strict '<', like KnnResult::push).
 * indices_dev int[nq][k] (-1 padded), sq_dists_dev double[nq][k] (may be NULL), num_found_dev int[nq] (may be NULL). Asynchronous. */
int gp_knn_search(const gp_point_grid_t* grid, const float* queries_dev, int num_queries, int k, double max_sq_dist, int* indices_dev, double* sq_dists_dev,
                  int* num_found_dev, gp_stream_t stream);
/* estimate_covariances(points, n, k): k-NN incl. the query -> sample covariance -> V diag(1e-3,1,1) V^-1; fewer than k -> identity.
 * covs_dev float[n][9] column-major; cell_size <= 0 picks 0.25 m; *num_short = points with < k neighbours. Synchronous.
 * How far an output is determined (tests/knn_ref.py holds every point to it): with l1 <= l2 <= l3 the eigenvalues of the sample covariance and
 * relgap = (l2 - l1) / l3, the output agrees with I - 0.999 v v^T (v: eigenvector of l1) to 1.5e-7 + 5.6e-7 / relgap in relative Frobenius norm.  Below
 * relgap 1e-6 -- collinear neighbours, and EVERY point at k = 2, whose sample covariance is rank one -- v is some unit vector of the plane of the two
 * smallest eigenvectors: which one is decided by the rounding noise of the uncentred sums, here as in the reference, so two correct implementations agree
 * there only as far as their roundings do.  The eigenvalues of the output are (1e-3, 1, 1) to 1e-5 always.  k = 1 gives diag(1e-3, 1, 1) exactly.  Among
 * neighbours at exactly the same distance at rank k either may be taken. */
int gp_estimate_covariances(const float* points_dev, int num_points, int k, double cell_size, float* covs_dev, int* num_short, gp_stream_t stream);
/* as above with a GP_TUNE_KNN_STRUCTURE value and (measurement) a device buffer of 8 work counters or NULL, see gp_point_grid_create_ex */
int gp_estimate_covariances_ex(const float* points_dev, int num_points, int k, double cell_size, float* covs_dev, int* num_short, int structure,
                               unsigned long long* counters_dev, gp_stream_t stream);
/* estimate_normals(points, covs, n), features/normal_estimation.cpp:18-50: n_i = the eigenvector of the smallest eigenvalue of covs_dev[i] (computeDirect, lower
 * triangle), turned round when p_i . n_i > 1 (points in the sensor frame: towards the origin once the tangent plane passes more than 1 m from it).
 * normals_dev float[n][3], f64 arithmetic rounded once at the store.  Within |p . n| <= 1 the sign is whatever the closed-form solver gives.  Asynchronous. */
int gp_estimate_normals_from_covs(const float* points_dev, const float* covs_dev, int num_points, float* normals_dev, gp_stream_t stream);
/* ONE k-NN search, both outputs: estimate_normals(points, n, k) (:52-55) and/or estimate_covariances.
 * normals_dev / covs_dev: either may be NULL, not both.  cell_size, *num_short, synchronous: as gp_estimate_covariances.  covs_dev is bit-identical to what
 * gp_estimate_covariances writes.  The normal is the eigenvector of the smallest eigenvalue of the sample covariance (which IS that of the regularised one),
 * determined like the covariance: sin of the angle to the true one <= (1.5e-7 + 5.6e-7 / relgap) / (0.999 sqrt 2).  Fewer than k neighbours or a non-finite
 * point: (+-1, 0, 0).  With normals_dev only, the V diag(1e-3,1,1) V^-1 products are skipped. */
int gp_estimate_normals_covariances(const float* points_dev, int num_points, int k, double cell_size, float* normals_dev, float* covs_dev, int* num_short,
                                    gp_stream_t stream);

typedef struct gp_gicp_factor gp_gicp_factor_t;
/* IntegratedGICPFactor(target, source) with its target 1-NN structure; max_correspondence_distance_sq defaults to 1.0 upstream (:30).
 * The factor owns that structure and an int per source point for the correspondences; both are allocated here, so a create that cannot
 * have the index array fails with the allocator's status (there is no slower kernel without it to fall back to later). */
int gp_gicp_factor_create(const float* target_points_dev, const float* target_covs_dev, int num_target, const float* points_dev, const float* covs_dev, int num_points,
                          double max_correspondence_distance_sq, gp_stream_t stream, gp_gicp_factor_t** out);
int gp_gicp_factor_create_ex(const float* target_points_dev, const float* target_covs_dev, int num_target, const float* points_dev, const float* covs_dev, int num_points,
                             double max_correspondence_distance_sq, int structure, unsigned long long* counters_dev, gp_stream_t stream, gp_gicp_factor_t** out);
int gp_gicp_factor_destroy(gp_gicp_factor_t* f);
int gp_gicp_factor_linearize(gp_gicp_factor_t* f, const double pose[16], gp_linearized6* out_host);           /* update_correspondences + evaluate */
/* evaluate(delta_eval) on the correspondences and Mahalanobis matrices of pose_lin.  The correspondences of the last linearise (or error
 * evaluation) are kept on the device: when pose_lin is bit for bit the pose they were computed at they are re-used -- the reference's
 * error() likewise evaluates on the stored correspondences (impl/integrated_gicp_factor_impl.hpp:183-185) -- otherwise the search runs
 * again at pose_lin.  gp_gicp_factor_linearize always searches, as update_correspondences does with its default (zero) tolerances. */
int gp_gicp_factor_compute_error(gp_gicp_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host);

/* IntegratedICPFactor_ (factors/integrated_icp_factor.hpp, impl/integrated_icp_factor_impl.hpp): point-to-point, or point-to-plane with the reference's
 * element-wise residual r = n_B o (mu_B - T p) (:210-213, :228-232), on the 1-NN correspondences of T_lin p with squared distance < max (:146-157; the
 * search and the transform in f64 on the f32 inputs).  error = sum r^T r (no 1/2, :215), H = sum J^T J, b = sum J^T r with J_t = diag(n_B) [-[q]x, I],
 * J_s = diag(n_B) [R [p]x, -R], R the pose's 3x3 block as given (:220-238).  Two linearises at one pose are bit-identical.
 * `grid` is BORROWED: a search structure over target_points_dev that the caller keeps alive for as long as the factor lives -- the reference's
 * target_tree argument (:47-51), many factors against one target share one.  target_normals_dev may be NULL unless point_to_plane (then
 * GP_ERROR_INVALID_ARGUMENT).  max_correspondence_distance_sq defaults to 1.0 upstream (:30). */
typedef struct gp_icp_factor gp_icp_factor_t;
int gp_icp_factor_create(const gp_point_grid_t* grid, const float* target_points_dev, const float* target_normals_dev, int num_target, const float* points_dev,
                         int num_points, double max_correspondence_distance_sq, int point_to_plane, gp_stream_t stream, gp_icp_factor_t** out);
int gp_icp_factor_destroy(gp_icp_factor_t* f); /* leaves the grid alone */
/* update_correspondences(delta) + evaluate (:128-248).  With the default (zero) tolerances every linearise searches. */
int gp_icp_factor_linearize(gp_icp_factor_t* f, const double pose[16], gp_linearized6* out_host);
/* evaluate(delta_eval) on the stored correspondences when pose_lin is bit for bit the pose of the last linearise or the pose they were searched at
 * (the reference's error() never searches once correspondences exist, :188-190); otherwise the search runs again at pose_lin. */
int gp_icp_factor_compute_error(gp_icp_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host);
/* set_correspondence_update_tolerance(angle, trans) (:128-141): with either > 0 and correspondences stored, a linearise at delta keeps them when the
 * rotation angle of delta^-1 * last_correspondence_point is < angle AND the norm of its translation is < trans (both strict: with one of the two left at
 * zero the search always runs); otherwise it searches and moves the correspondence point.  The decision is made on the host. */
int gp_icp_factor_set_correspondence_update_tolerance(gp_icp_factor_t* f, double angle, double trans);
/* source points that had a correspondence in the last linearise (= its record's num_inliers); 0 before one */
int gp_icp_factor_num_correspondences(const gp_icp_factor_t* f);

/* IntegratedPointToEdgeFactor_, IntegratedPointToPlaneFactor_ and IntegratedLOAMFactor_ (factors/integrated_loam_factor.hpp, impl/integrated_loam_factor_impl.hpp) in
 * one handle: an edge part and a plane part, either of which may be absent (grid NULL and both counts 0).  Both grids are BORROWED, as for gp_icp_factor_create: the
 * reference's target_edges_tree / target_planes_tree.  Neither part: GP_ERROR_INVALID_ARGUMENT; a part with a grid but NULL points likewise.
 *   correspondences  per source point the K nearest target points of T_lin p (f64 on the f32 inputs) with squared distance < max, in ascending order of distance,
 *                    K = 2 (edge, :235-279) or 3 (plane, :80-124); fewer than K within the cut-off: no correspondence.  Index 0 is the anchor x_j.
 *   edge  (:300-365) v = x_j - x_l, c = 1/|v|, r = c (q - x_j) x (q - x_l) = A d with A = c [v]x, d = x_j - q, q = T p: error = d^T M d, H = sum J^T M J,
 *                    b = sum J^T M d with M = A^T A = c^2 [v]x^T [v]x and J_t = [-[q]x, I], J_s = [R [p]x, -R] as for ICP.
 *   plane (:127-194) n = normalize((x_j - x_l) x (x_j - x_m)), r = n o (x_j - q) element-wise: the point-to-plane ICP term with M = diag(n o n).
 *                    M, c and n are formed in f64 from the f32 target points.  Degenerate neighbours (x_j = x_l, a collinear triple) are NOT guarded, as in the
 *                    reference: the division yields non-finite values that flow into the sums, and the call still returns GP_OK.
 *   validation       IntegratedLOAMFactor_::validate_correspondences (:487-529), off by default; a kernel behind the searches whenever it is enabled (also when the
 *                    tolerances kept the correspondences: it is idempotent).  theta(p) = atan2(p.z, hypot(p.x, p.y)) in f64; an edge pair is dropped when
 *                    |theta_j - theta_l| < 0.1 pi / 180, a plane triple when that holds and |theta_j - theta_m| < 0.1 * pi * 180.
 *                    The second bound is the reference's expression as written (about 56.5 rad, so it always holds); parity with the reference is the target.
 *   record           the edge part's finalised record plus the plane part's, added in that order in f64 (IntegratedLOAMFactor_::evaluate, :461-472);
 *                    num_inliers is the sum of the two counts.  Two linearises at one pose are bit-identical.
 * set_max_correspondence_distance takes DISTANCES (squared inside; default 1.0 each, :27, :205; must be positive); it does not touch stored correspondences.
 * set_correspondence_update_tolerance is gp_icp_factor_set_correspondence_update_tolerance's host rule, applied to both parts.  compute_error has the semantics of
 * gp_icp_factor_compute_error: on the stored correspondences when pose_lin is bit for bit the pose of the last linearise or search, otherwise it searches at pose_lin.
 * Every entry point refuses a NULL handle on the host, before any device work. */
typedef struct gp_loam_factor gp_loam_factor_t;
int gp_loam_factor_create(const gp_point_grid_t* edge_grid, const float* target_edges_dev, int num_target_edges, const float* source_edges_dev, int num_source_edges,
                          const gp_point_grid_t* plane_grid, const float* target_planes_dev, int num_target_planes, const float* source_planes_dev, int num_source_planes,
                          gp_stream_t stream, gp_loam_factor_t** out);
int gp_loam_factor_destroy(gp_loam_factor_t* f); /* leaves the grids alone */
int gp_loam_factor_set_max_correspondence_distance(gp_loam_factor_t* f, double dist_edge, double dist_plane);
int gp_loam_factor_set_enable_correspondence_validation(gp_loam_factor_t* f, int on);
int gp_loam_factor_set_correspondence_update_tolerance(gp_loam_factor_t* f, double angle, double trans);
int gp_loam_factor_linearize(gp_loam_factor_t* f, const double pose[16], gp_linearized6* out_host);
int gp_loam_factor_compute_error(gp_loam_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host);
/* source points that had a correspondence in the last linearise, per part (either pointer may be NULL); 0 before one */
int gp_loam_factor_num_correspondences(const gp_loam_factor_t* f, int* edges, int* planes);
/* read-only copy of the stored correspondences (of the last search, behind the validation when it is enabled) to the host, for tests and diagnosis: edges_host
 * int[2][num_source_edges], planes_host int[3][num_source_planes], slot k of source point i at [k * n + i], every slot -1 where the point has none.  Either pointer
 * may be NULL; an absent or empty part writes nothing.  Synchronous.  GP_ERROR_INVALID_ARGUMENT before the first linearise / error evaluation. */
int gp_loam_factor_get_correspondences(const gp_loam_factor_t* f, int* edges_host, int* planes_host);

/* IntensityGradients::estimate (factors/intensity_gradients.cpp:20-133): per point i with normal n and intensity I, over the slots j = 1 .. k-1 of its k-NN list
 * (slot 0 is the point itself and is skipped, :54, :100): row 0 of A is n with b_0 = 0 (:50-51, :96-97), row j is (p_j - ((p_j - p) . n) n) - p with
 * b_j = I_j - I (:58-60, :104-106); H = A^T A, e = A^T b, g = H^-1 e (:63-65, :109-111).  f64 on the f32 inputs, the closed-form cofactor inverse, rounded once at
 * the store into gradients_dev float[n][3].  A singular H is NOT guarded, as in the reference: its non-finite values are stored and the call returns GP_OK.
 * _from_neighbors is the overload on a given neighbour table (:20-69): neighbors_dev int[n][k], of which the first k_photo slots are used, 1 <= k_photo <= k
 * (:32-35).  A point with a slot among those that is no point index (the -1 padding of gp_knn_search; anything outside [0, n)) gets (0, 0, 0).  Asynchronous.
 * gp_estimate_intensity_gradients (:71-133) builds a search structure, runs gp_knn_search (1 <= k <= 32) into a temporary table and takes all k slots:
 * cell_size <= 0 picks 0.25 m and *num_short (may be NULL) is the number of points with fewer than k neighbours, as for gp_estimate_covariances; those points get
 * (0, 0, 0).  Synchronous.  Both refuse a NULL array with GP_ERROR_INVALID_ARGUMENT before any device work.
 * The reference's third entry (:135-242: normals, covariances and gradients from one search) is not provided: it turns a normal round at n . p > 0, a rule
 * gp_estimate_normals_* (p . n > 1) does not share. */
int gp_estimate_intensity_gradients_from_neighbors(const float* points_dev, const float* normals_dev, const float* intensities_dev, int num_points,
                                                   const int* neighbors_dev, int k, int k_photo, float* gradients_dev, gp_stream_t stream);
int gp_estimate_intensity_gradients(const float* points_dev, const float* normals_dev, const float* intensities_dev, int num_points, int k, double cell_size,
                                    float* gradients_dev, int* num_short, gp_stream_t stream);

/* IntegratedColoredGICPFactor_ (factors/integrated_colored_gicp_factor.hpp, impl/integrated_colored_gicp_factor_impl.hpp) on the 1-NN correspondences of T_lin p
 * with squared distance < max (:119-129; the 3-D search of the other factors, or -- gp_colored_gicp_factor_set_intensity_grid below -- the reference's 4-D
 * IntensityKdTree search, in which the distance held against max is the 4-D one).  With q = T p_A,
 * d = mu_B - q, P = I - n_B n_B^T and u = P g_B (g_B the target's intensity gradient, :236-241):
 *   geometric    d with M_g = (C_B + R C_A R^T)^-1 taken at the LINEARISATION pose, as update_correspondences stores it (:134-138)
 *   photometric  r_p = I_B - I_A - u . d (:207-209)
 *   w_p = photometric_term_weight (default 0.25 upstream, :29), w_g = 1 - w_p (:174)
 *   error = sum w_g d^T M_g d + w_p r_p^2 (:204, :211; no 1/2), H = sum J^T M J with M = w_g M_g + w_p u u^T (:229-231, :246-248),
 *   b = sum J^T w with w = w_g M_g d - w_p r_p u (:232-233, :249-250), J_t = [-[q]x, I], J_s = [R [p]x, -R], R the pose's 3x3 block as given.
 *   (The reference writes q - mu_B and J = [[q]x, -I], :203, :217-223: the products are the same.)
 * `grid` is BORROWED, as for gp_icp_factor_create.  create returns GP_ERROR_INVALID_ARGUMENT, before any device work, for a NULL grid or array and for a weight
 * outside [0, 1].  linearize / compute_error / set_correspondence_update_tolerance / num_correspondences have the semantics of their gp_icp_factor_* namesakes:
 * compute_error evaluates on the stored correspondences when pose_lin is bit for bit the pose of the last linearise or search.  set_max_correspondence_distance
 * takes a DISTANCE (squared inside; must be positive) and leaves stored correspondences alone.  Every entry point refuses a NULL handle on the host.  Two
 * linearises at one pose are bit-identical. */
typedef struct gp_colored_gicp_factor gp_colored_gicp_factor_t;
int gp_colored_gicp_factor_create(const gp_point_grid_t* grid, const float* target_points_dev, const float* target_covs_dev, const float* target_normals_dev,
                                  const float* target_intensities_dev, const float* target_gradients_dev, int num_target, const float* points_dev,
                                  const float* covs_dev, const float* intensities_dev, int num_points, double max_correspondence_distance_sq,
                                  double photometric_term_weight, gp_stream_t stream, gp_colored_gicp_factor_t** out);
int gp_colored_gicp_factor_destroy(gp_colored_gicp_factor_t* f); /* leaves the grid alone */
int gp_colored_gicp_factor_linearize(gp_colored_gicp_factor_t* f, const double pose[16], gp_linearized6* out_host);
int gp_colored_gicp_factor_compute_error(gp_colored_gicp_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host);
int gp_colored_gicp_factor_set_photometric_term_weight(gp_colored_gicp_factor_t* f, double weight);
int gp_colored_gicp_factor_set_max_correspondence_distance(gp_colored_gicp_factor_t* f, double dist);
int gp_colored_gicp_factor_set_correspondence_update_tolerance(gp_colored_gicp_factor_t* f, double angle, double trans);
int gp_colored_gicp_factor_num_correspondences(const gp_colored_gicp_factor_t* f);

/* IntensityKdTree (ann/intensity_kdtree.hpp, src/gtsam_points/ann/intensity_kdtree.cpp): exact 1-NN in (x, y, z, intensity).  For a query (q, I_q) the answer is the
 * target index j that minimises
 *     d4^2(j) = |q - x_j|^2 + (I_q - s I_j)^2,   s = intensity_scale,
 * the scale on the STORED side only, as the reference writes it (kdtree_get_pt multiplies by intensity_scale; the factors put the raw source intensity into pt[3]).
 * f64 on the f32 inputs (s I_j one f64 product); a match is kept when d4^2 < max_sq_dist (strict; the reference's knn_search ignores max_sq_dist and its callers
 * apply this test).  Ties: the LOWEST target index among the nearest.  Same bits on every run.
 * The structure is a gp_point_grid over the points (cell_size <= 0 picks 0.25 m; the binned grid, or the hashed one for a bounding box too wide for it) plus a
 * cell-sorted copy of the intensities; it OWNS those and BORROWS points_dev / intensities_dev, which must outlive it unchanged.
 * Deviations: k = 1 only and no search_eps (the approximate search).  A target point with a non-finite coordinate or intensity is never matched and a query with
 * one gets -1 (nanoflann's behaviour on NaN is unspecified).  As with gp_knn_search, an unbounded query (max_sq_dist = DBL_MAX) far from every point walks the
 * structure until its bounding box is exhausted.
 * gp_intensity_grid_search: queries_dev double[m][4] = (x, y, z, intensity) -> indices_dev int[m] (-1: none), sq_dists_dev double[m] (may be NULL; max_sq_dist where
 * there is none).  Asynchronous on `stream`.  create is synchronous.  destroy synchronises the device. */
typedef struct gp_intensity_grid gp_intensity_grid_t;
int gp_intensity_grid_create(const float* points_dev, const float* intensities_dev, int num_points, double intensity_scale, double cell_size, gp_stream_t stream,
                             gp_intensity_grid_t** out);
int gp_intensity_grid_destroy(gp_intensity_grid_t* g);
int gp_intensity_grid_search(const gp_intensity_grid_t* g, const double* queries_dev, int m, double max_sq_dist, int* indices_dev, double* sq_dists_dev, gp_stream_t stream);
/* the 3-D structure inside (owned by `g`, valid while it lives): what a factor's create takes as `grid` before _set_intensity_grid hands it `g`; NULL for NULL */
const gp_point_grid_t* gp_intensity_grid_point_grid(const gp_intensity_grid_t* g);
/* from now on the factor's correspondence pass is the XYZI search on `xyzi` (BORROWED; built over the factor's target points and intensities) with the source's
 * intensities as I_q, integrated_colored_gicp_factor_impl.hpp:121-127; NULL: back to the 3-D grid.  Stored correspondences are forgotten.  A factor in this state is
 * refused by gp_corr_batch_create* (the batch searches in 3-D). */
int gp_colored_gicp_factor_set_intensity_grid(gp_colored_gicp_factor_t* f, const gp_intensity_grid_t* xyzi);

/* IntegratedColorConsistencyFactor_ (factors/integrated_color_consistency_factor.hpp, impl/integrated_color_consistency_factor_impl.hpp): the photometric term of
 * the colored GICP factor alone, on the 1-NN correspondences of T_lin p (3-D on `grid`, or XYZI after _set_intensity_grid).  With q = T p_A, d = mu_B - q,
 * u = (I - n_B n_B^T) g_B, r_p = I_B - I_A - u . d and w = photometric_term_weight (default 1.0 upstream, :31; any finite w >= 0):
 *   error = sum w r_p^2 (:200; no 1/2), H = sum J^T (w u u^T) J (:217-219), b = sum J^T (-w r_p u) (:220-221), J_t = [-[q]x, I], J_s = [R [p]x, -R].
 * No covariance is read.  `grid` is BORROWED.  Every entry point has the semantics of its gp_colored_gicp_factor_* namesake.  Not a member of gp_corr_batch_* yet. */
typedef struct gp_color_consistency_factor gp_color_consistency_factor_t;
int gp_color_consistency_factor_create(const gp_point_grid_t* grid, const float* target_points_dev, const float* target_normals_dev, const float* target_intensities_dev,
                                       const float* target_gradients_dev, int num_target, const float* points_dev, const float* intensities_dev, int num_points,
                                       double max_correspondence_distance_sq, double photometric_term_weight, gp_stream_t stream, gp_color_consistency_factor_t** out);
int gp_color_consistency_factor_destroy(gp_color_consistency_factor_t* f); /* leaves the grids alone */
int gp_color_consistency_factor_set_intensity_grid(gp_color_consistency_factor_t* f, const gp_intensity_grid_t* xyzi);
int gp_color_consistency_factor_linearize(gp_color_consistency_factor_t* f, const double pose[16], gp_linearized6* out_host);
int gp_color_consistency_factor_compute_error(gp_color_consistency_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host);
int gp_color_consistency_factor_set_photometric_term_weight(gp_color_consistency_factor_t* f, double weight);
int gp_color_consistency_factor_set_max_correspondence_distance(gp_color_consistency_factor_t* f, double dist);
int gp_color_consistency_factor_set_correspondence_update_tolerance(gp_color_consistency_factor_t* f, double angle, double trans);
int gp_color_consistency_factor_num_correspondences(const gp_color_consistency_factor_t* f);

/* IntegratedCT_ICPFactor_ / IntegratedCT_GICPFactor_ (factors/integrated_ct_icp_factor.hpp, integrated_ct_gicp_factor.hpp and their impl/ files): a scan taken
 * while the sensor moved from pose0 (first key) to pose1 (second key), every source point transformed by the pose interpolated at its own time stamp.
 *   time table   built once, at create, on the host from times_dev (:41-55): in index order a new entry opens when t - table.back() > 1e-3 (strict; f64 on the f32
 *                times), time_index[i] is the last entry at that moment, then every entry is divided by max(1e-9, table.back()).  No sort, no offset.
 *   pose table   per call (update_poses, :202-248), GTSAM's Pose3 conventions (tangent (omega, v), right-trivialised derivatives), f64: for each entry t
 *                delta = pose0^-1 pose1, vel = Log(delta), inc = Exp(t vel), T(t) = pose0 inc,
 *                D0(t) = Ad(inc^-1) - t Jr(t vel) Jr^-1(vel) Ad(delta^-1), D1(t) = t Jr(t vel) Jr^-1(vel); small angles by series (pose0 == pose1 included).
 *   search       the nearest target point of T(t_i) p_i with squared distance < max (strict, as gp_icp_factor_*), f64 on the f32 inputs.
 *   per point    J = R(t_i) [-[p]x, I];  kind 0 (CT-ICP): the scalar e = n_B . (T p - x_B), H_a = n_B^T J D_a, error += e^2 (no 1/2);
 *                kind 1 (CT-GICP): r = T p - x_B, H_a = J D_a, M = (C_B + R(t_i) C_A R(t_i)^T)^-1 of the LINEARISATION poses, error += r^T M r.
 *   record       gp_linearized6 over (pose0, pose1): H_target = H_00 = sum H_0^T M H_0, H_source = H_11, H_target_source = H_01, b_target = b_0 = sum H_0^T M r,
 *                b_source = b_1, error, num_inliers = matched points.  The reference's HessianFactor is (k0, k1, H_00, H_01, -b_0, H_11, -b_1, error).
 * `grid` is BORROWED, as for gp_icp_factor_create.  create copies the times to the host once; it returns GP_ERROR_INVALID_ARGUMENT before any device work for a
 * NULL grid, points or times, kind 0 without target normals, kind 1 without either covariance array, a kind that is neither, and a negative cut-off.
 * linearize always searches.  compute_error evaluates on the stored correspondences (kind 1: with M of the stored linearisation pose table) and searches at the
 * given poses only when nothing is stored (:92-96).  deskew writes T(t_i) p_i -- T0^-1 T(t_i) p_i when `local` -- as double[num_points][4], last component 1
 * (:290-308).  All are synchronous; two linearises at the same poses are bit-identical.  num_points == 0: a zero record, error 0.
 * For tests and callers: the number of table entries; the table (double[bins]) and the indices (int[num_points]); the pose table of the last linearise (or
 * first error evaluation), double[bins][12 + 36 + 36] = T(t) 3x4 | D0 | D1, all row-major; the stored correspondences, int[num_points], -1 = none.  The last
 * two return GP_ERROR_INVALID_ARGUMENT before anything is stored. */
typedef struct gp_ct_factor gp_ct_factor_t;
int gp_ct_factor_create(const gp_point_grid_t* grid, const float* target_points_dev, const float* target_normals_dev, const float* target_covs_dev, int num_target,
                        const float* points_dev, const float* covs_dev, const float* times_dev, int num_points, double max_correspondence_distance_sq,
                        int kind /* 0 ICP, 1 GICP */, gp_stream_t stream, gp_ct_factor_t** out);
int gp_ct_factor_destroy(gp_ct_factor_t* f); /* leaves the grid alone */
int gp_ct_factor_linearize(gp_ct_factor_t* f, const double pose0[16], const double pose1[16], gp_linearized6* out_host);
int gp_ct_factor_compute_error(gp_ct_factor_t* f, const double pose0[16], const double pose1[16], double* out_host);
int gp_ct_factor_deskew(gp_ct_factor_t* f, const double pose0[16], const double pose1[16], int local, double* out_dev);
int gp_ct_factor_num_time_bins(const gp_ct_factor_t* f);
int gp_ct_factor_time_table(const gp_ct_factor_t* f, double* table_host, int* indices_host);
int gp_ct_factor_pose_table(gp_ct_factor_t* f, double* out_host);
int gp_ct_factor_correspondences(gp_ct_factor_t* f, int* out_host);

/* ---- a batch of GICP / ICP / LOAM / colored GICP factors with the relative poses in DEVICE memory (gp_corr_batch.hip) ----
 * What gp_vgicp_batch_issue_linearize_dev / _issue_compute_error_dev are to the VGICP factor: any number of the factors above linearised (or evaluated) in a number of
 * launches that does not depend on their count -- one search launch, one tile launch per factor kind present (GICP, ICP point-to-point, ICP point-to-plane), one
 * finalize launch --, the poses read from a table double[F][16] (column-major) in device memory.  The batch BORROWS the factor handles (the caller keeps them and
 * their clouds alive) and keeps correspondences of its own: a batch pass does not touch what the factors' own calls store, and the other way round.
 *   record order  the GICP factors in the order given, then the ICP factors in the order given: pose f, record f and error f belong to member f.
 *   create        GP_ERROR_INVALID_ARGUMENT for: a NULL handle, a factor created on another stream than `stream`, an empty batch (num_gicp + num_icp = 0), an ICP factor
 *                 whose correspondence-update tolerances are not both zero (that keep-or-search decision is host logic on a host pose; in a batch every linearise
 *                 searches: the reference's default for both factor types).
 *   sets          the batch holds TWO sets of correspondences, set 0 and set 1.  A linearise searches every member's correspondences at its pose INTO the set it names
 *                 and sums on them; an error evaluation reads the set it names and never searches -- the reference's error(), which evaluates on the correspondences
 *                 of the last linearise.  So a caller that linearises ahead (gp_lm_graph_*: at a trial's values, into the other set) still evaluates further trials on
 *                 the correspondences of its linearisation point.  Evaluating a set that was never linearised: GP_ERROR_INVALID_ARGUMENT.
 *   rigid         as gp_vgicp_batch_issue_linearize_dev: 1 = the caller vouches that every 3x3 block is orthonormal to 1e-9 (29 sums + adjoint expansion, what the
 *                 factors' own calls choose for such a pose), 0 = the 92 explicit sums with J_s from the block as given.
 *   bits          a record / an error equals, bit for bit, that of the member's own gp_*_factor_linearize / _compute_error at the same pose(s) (same terms, same
 *                 1024-point tiles, same order of sums).  A member without points, or none of whose points has a target within the cut-off: an all-zero record, error 0.
 * The issue_ forms are asynchronous on the batch's stream.  issue_compute_error_dev: out [F] may be device or host-mapped memory; done_flags (may be NULL) = F words of
 * host-mapped memory, word f receives done_seq behind error f (for a caller that polls instead of synchronising the stream).
 * gp_corr_batch_linearize / _compute_error: the synchronous host-pose forms on set 0 (poses up, wait, results down); compute_error evaluates on the correspondences of
 * the last linearise into set 0, with poses_lin the poses of that linearise (GICP's fused covariances are taken at them).
 * gp_corr_batch_create_ex adds LOAM members (gp_corr_batch_create means num_loam = 0); record order GICP, ICP, then LOAM, each in the order given.  A LOAM member with
 * non-zero update tolerances is refused like an ICP one; validation is allowed and runs as a kernel behind the search launch, into the set being written.  A member's
 * cut-offs and validation switch are read when the batch is created.  Launches with LOAM members: one more search launch (the K > 1 parts), one tile launch per term
 * kind present (edge, plane), the validation launch if any member enables it, one finalize over the PARTS, and -- when a member has both parts -- one launch that
 * hands each member its pose in front and one that adds the edge part's record and the plane part's in that order in f64 behind: a LOAM member's record and error
 * equal, bit for bit, those of gp_loam_factor_linearize / _compute_error at the same pose(s), in both sets.
 * gp_corr_batch_create_ex2 adds colored GICP members (gp_corr_batch_create_ex means num_colored = 0); record order GICP, ICP, LOAM, then colored GICP, each in the
 * order given, so a batch of the older kinds keeps its order.  A colored member is a 1-NN kind like GICP: the one search launch of the GICP / ICP members searches it
 * too, and it adds one tile launch per pass (the single factor's term from a descriptor table of its own) and nothing else, whatever the number of members.  Its
 * record and error equal, bit for bit, those of gp_colored_gicp_factor_linearize / _compute_error at the same pose(s), in both sets (M_g at poses_lin, d and the
 * photometric residual at poses_eval).  A member's photometric_term_weight and max_correspondence_distance are read when the batch is created: a later
 * gp_colored_gicp_factor_set_photometric_term_weight / _set_max_correspondence_distance does not reach an existing batch.  Refused with GP_ERROR_INVALID_ARGUMENT: a
 * NULL handle, a colored factor created on another stream, one whose correspondence-update tolerances are not both zero (as for ICP and LOAM). */
typedef struct gp_corr_batch gp_corr_batch_t;
int gp_corr_batch_create(const gp_gicp_factor_t* const* gicp, int num_gicp, const gp_icp_factor_t* const* icp, int num_icp, gp_stream_t stream, gp_corr_batch_t** out);
int gp_corr_batch_create_ex(const gp_gicp_factor_t* const* gicp, int num_gicp, const gp_icp_factor_t* const* icp, int num_icp, const gp_loam_factor_t* const* loam, int num_loam,
                            gp_stream_t stream, gp_corr_batch_t** out);
int gp_corr_batch_create_ex2(const gp_gicp_factor_t* const* gicp, int num_gicp, const gp_icp_factor_t* const* icp, int num_icp, const gp_loam_factor_t* const* loam, int num_loam,
                             const gp_colored_gicp_factor_t* const* colored, int num_colored, gp_stream_t stream, gp_corr_batch_t** out);
int gp_corr_batch_destroy(gp_corr_batch_t* batch); /* synchronises the batch's stream; leaves the factors alone */
int gp_corr_batch_size(const gp_corr_batch_t* batch);
int gp_corr_batch_stream(const gp_corr_batch_t* batch, gp_stream_t* out);
int gp_corr_batch_sync(gp_corr_batch_t* batch);
int gp_corr_batch_issue_linearize_dev(gp_corr_batch_t* batch, const double* poses_dev, int rigid, int set, gp_linearized6* out_dev);
int gp_corr_batch_issue_compute_error_dev(gp_corr_batch_t* batch, int set, const double* poses_lin_dev, const double* poses_eval_dev, double* out,
                                          unsigned long long* done_flags, unsigned long long done_seq);
int gp_corr_batch_linearize(gp_corr_batch_t* batch, const double* poses_host, int rigid, gp_linearized6* out_host);
int gp_corr_batch_compute_error(gp_corr_batch_t* batch, const double* poses_lin_host, const double* poses_eval_host, double* out_host);

/* ---- the step after the path: damped normal equations assembled and solved on the device ----
 * DenseLinearSystemBuilder (optimizers/linear_system_builder.cpp:39-48): A = sum of the Hessian blocks scattered by key,
 *   b = sum of g (= -b_target / -b_source, integrated_matching_cost_factor.cpp:49), c = sum of the errors;
 * buildDampedSystem (optimizers/levenberg_marquardt_ext.cpp:146-161): A + lambda I, or A + lambda clamp(diag A, min, max);
 * DenseLinearSolver::solve(A, b) (optimizers/linear_solver.hpp:18-22): A x = b, here by a blocked LL^T in f64.
 * Variables are 6-dof poses in num_slots slots; factor_slots = [num_factors][2] = (target slot, source slot), a negative
 * slot = a pose that is not a variable (fixed / unary factor).  records_dev = the stacked [num_factors] gp_linearized6
 * records exactly as gp_vgicp_batch_issue_linearize (or the multi-GPU all-reduce) leaves them in HBM. */
typedef struct gp_dense_system gp_dense_system_t;
int gp_dense_system_create(int num_slots, const int* factor_slots, int num_factors, gp_stream_t stream, gp_dense_system_t** out);
int gp_dense_system_destroy(gp_dense_system_t* sys);
int gp_dense_system_size(const gp_dense_system_t* sys); /* 6 * num_slots */
/* prior_diag_host: optional [6 * num_slots] extra diagonal (prior factors), may be NULL */
int gp_dense_system_build(gp_dense_system_t* sys, const gp_linearized6* records_dev, double lambda, int diagonal_damping, double min_diagonal, double max_diagonal,
                          const double* prior_diag_host);
/* A as a full symmetric column-major [n][n], b [n], c; any pointer may be NULL.  Synchronous. */
int gp_dense_system_download(const gp_dense_system_t* sys, double* A_host, double* b_host, double* c_host);
/* x (host and / or device copy, either may be NULL); consumes the built system.  GP_ERROR_INDETERMINATE if not positive definite. */
int gp_dense_system_solve(gp_dense_system_t* sys, double* x_host, double* x_dev);
/* One damped step of the optimizer's inner loop (LevenbergMarquardtOptimizerExt::tryLambda: buildDampedSystem + solve, optimizers/levenberg_marquardt_ext.cpp:146-161, 200-220)
 * as ONE call with ONE synchronisation (the dense form with a prior_diag_host: two): build + download(b, c) + solve, bit-identical to the three calls.  x_host [n], b_host [n] (the undamped gradient side the optimizer's
 * model-fidelity test needs), c_host [1]; any may be NULL.  GP_ERROR_INDETERMINATE if not positive definite: b_host / c_host are valid, x_host is not written. */
int gp_dense_system_step(gp_dense_system_t* sys, const gp_linearized6* records_dev, double lambda, int diagonal_damping, double min_diagonal, double max_diagonal,
                         const double* prior_diag_host, double* x_host, double* b_host, double* c_host);

/* gp_dense_system_step in two halves: issue queues the step's kernels on the system's stream and returns; finish waits for the stream and hands over x / b / c
 * (GP_ERROR_INDETERMINATE as the one call).  Work queued on the same stream between the two -- a consumer of the solution where the step leaves it ON THE DEVICE
 * (gp_dense_system_device_solution: x [n] in slot order, the status word: != 0 = indeterminate, x is not to be used) -- shares the step's one wait (gp_lm_graph_try_lambda). */
int gp_dense_system_issue_step(gp_dense_system_t* sys, const gp_linearized6* records_dev, double lambda, int diagonal_damping, double min_diagonal, double max_diagonal,
                               const double* prior_diag_host);
int gp_dense_system_finish_step(gp_dense_system_t* sys, double* x_host, double* b_host, double* c_host);
/* (one step in flight per system: an issue before the last one was finished or collected fails with GP_ERROR_INVALID_ARGUMENT and leaves that step untouched) */
int gp_dense_system_device_solution(gp_dense_system_t* sys, const double** x_dev, const int** status_dev);
/* a system of ONE pose (a scan registered onto a map) runs its step -- assembly, error sum, damping, 6 x 6 Cholesky, both substitutions, hand-over -- as ONE launch of one
 * 64-thread workgroup, the multi-launch path's arithmetic operation for operation (bit-identical); 0 selects the multi-launch path (tests, A/B); returns what the next
 * step runs (1 / 0).  A step with a prior_diag_host takes the multi-launch path. */
int gp_dense_system_set_one_launch(gp_dense_system_t* sys, int enable);
/* finish_step for a caller that has SEEN the stream pass the step (a completion word of work it queued behind the step): no wait of its own */
int gp_dense_system_collect_step(gp_dense_system_t* sys, double* x_host, double* b_host, double* c_host);

/* ---- the same step, block-sparse: SparseLinearSystemBuilder<6> + SparseLinearSolver ----
 * SparseLinearSystemBuilder<BLOCK_SIZE> (include/gtsam_points/optimizers/linear_system_builder.hpp:41-72): A as a lower-triangular
 *   block-sparse matrix in a given ordering, b, c;  SparseLinearSolver::solve(A, b) (optimizers/linear_solver.hpp:24-29), called from
 *   levenberg_marquardt_ext.cpp:200-220.  Here: 6x6 blocks in a block-column structure that already holds the fill of the factor,
 *   left-looking block LL^T in f64 scheduled over the elimination tree (independent subtrees = one workgroup each, then the
 *   separator columns), forward substitution fused, four launches per solve; every block is a gather in a fixed order (deterministic).
 * ordering: 0 = natural (the slot order is the elimination order: "the ordering from the factor key list"),
 *           1 = nested dissection by BFS bisection of the pose graph (shallow elimination tree: chains become ~log2(P) levels),
 *           2 = minimum degree by multiple elimination (the fill of a COLAMD-class ordering, which is what GTSAM gives the reference's solves:
 *               optimizers/levenberg_marquardt_ext.cpp:200-220); 3 = the same with a slack of one on the degree (more nodes per round: a bushier tree),
 *           4 = automatic: 1 and 3 are both tried, the schedule with the shorter critical path (then the smaller factor) is kept.
 * The numeric phase runs one launch per LEVEL of the schedule: the independent subtrees, then the chains of separator columns level by level.
 * Same slot / record conventions as gp_dense_system_*; no limit on num_slots. */
typedef struct gp_sparse_system gp_sparse_system_t;
int gp_sparse_system_create(int num_slots, const int* factor_slots, int num_factors, int ordering, gp_stream_t stream, gp_sparse_system_t** out);
int gp_sparse_system_destroy(gp_sparse_system_t* sys);
int gp_sparse_system_size(const gp_sparse_system_t* sys); /* 6 * num_slots */
/* structure: blocks of A (lower triangle incl. diagonal), blocks of L (incl. fill), 6x6 block products per factorisation,
 * independent subtrees, columns in the top part; any pointer may be NULL */
int gp_sparse_system_info(const gp_sparse_system_t* sys, int64_t* nnz_a_blocks, int64_t* nnz_l_blocks, int64_t* block_products, int* num_subtrees, int* top_columns);
int gp_sparse_system_build(gp_sparse_system_t* sys, const gp_linearized6* records_dev, double lambda, int diagonal_damping, double min_diagonal, double max_diagonal,
                           const double* prior_diag_host);
/* for checkers: A expanded to a full symmetric column-major [n][n] in slot order, b [n], c; any pointer may be NULL.  Synchronous. */
int gp_sparse_system_download(const gp_sparse_system_t* sys, double* A_host, double* b_host, double* c_host);
/* x in slot order (host and / or device copy, either may be NULL); consumes the built system.  GP_ERROR_INDETERMINATE if not positive definite. */
int gp_sparse_system_solve(gp_sparse_system_t* sys, double* x_host, double* x_dev);
/* gp_dense_system_step's block-sparse form, one wait.  The assembly kernel applies the damping and hands b, c to the host.  A system whose factor and index lists fit the
 * LDS of one compute unit (<= 128 poses, <= ~400 blocks of L: BASELINE configs[2]'s 64-pose graph does) is then factored and solved -- all levels, both substitutions, x
 * and status to the host -- by ONE launch of one 512-thread workgroup with every operand in LDS (sparse_small_step_kernel; a team of waves per work list that meets
 * through LDS words where a level has at most four lists -- no workgroup barrier inside a list --, else a lone wave per list / lock-step teams): two launches per step;
 * larger systems take 2 + 2 x levels launches.  The forms are bit-identical; gp_sparse_system_set_one_launch(sys, 0) selects the multi-launch form for a qualifying
 * system, 2 the one-launch step's first form (every list a team of waves in lock step), 3 its second (a lone wave per list throughout), 1 the default; returns what the
 * next step runs (0 / 2 / 3 / 1). */
int gp_sparse_system_step(gp_sparse_system_t* sys, const gp_linearized6* records_dev, double lambda, int diagonal_damping, double min_diagonal, double max_diagonal,
                          const double* prior_diag_host, double* x_host, double* b_host, double* c_host);
int gp_sparse_system_set_one_launch(gp_sparse_system_t* sys, int enable);
/* gp_sparse_system_step in two halves, as gp_dense_system_issue_step / _finish_step / _device_solution (prior_diag_host is copied by issue: the caller's array is free on return) */
int gp_sparse_system_issue_step(gp_sparse_system_t* sys, const gp_linearized6* records_dev, double lambda, int diagonal_damping, double min_diagonal, double max_diagonal,
                                const double* prior_diag_host);
int gp_sparse_system_finish_step(gp_sparse_system_t* sys, double* x_host, double* b_host, double* c_host);
int gp_sparse_system_device_solution(gp_sparse_system_t* sys, const double** x_slots_dev, const int** status_dev);
int gp_sparse_system_collect_step(gp_sparse_system_t* sys, double* x_host, double* b_host, double* c_host);
/* measurement hook: thread 0 of sparse_small_step_kernel stamps its phases (s_memtime) into dev_buffer (64 uint64: [0] start, [1] lists and system in LDS, [2] factored,
 * [3] substituted, [4] end, [8 + 4 r + 0..3] round r < 14 of the first level: start / gathered / diagonal block done / blocks below done); NULL = off */
int gp_debug_sparse_step_trace(gp_sparse_system_t* sys, unsigned long long* dev_buffer);
/* ---- one Levenberg-Marquardt trial without the host in the middle: the values live beside the records (gp_lm.hip) ----
 * The reference's optimizer (optimizers/levenberg_marquardt_ext.cpp) hands `values` to its GPU factor set twice per trial -- linearization_hook_->linearize(values)
 * (iterate(), :352-392 -> cuda/nonlinear_factor_set_gpu.cpp:64-101) and linearization_hook_->error(newValues) (tryLambda(), :245 -> :103-139) -- and retracts on the host
 * between them (:239).  A gp_lm_graph keeps the N poses in device memory: batch member i is the pairwise factor between poses pose_pairs[2 i] (target) and
 * pose_pairs[2 i + 1] (source) and is evaluated at target^-1 source (integrated_matching_cost_factor.cpp:28-31); pose_fixed[i] != 0 holds pose i (NULL = none held:
 * the gauge is then the caller's problem, the step reports GP_ERROR_INDETERMINATE); the free poses take the variable slots 0, 1, ... in pose order.  The graph builds
 * its own damped system on the batch's stream (one free pose: the dense 6 x 6 step; else block-sparse in `ordering`, gp_sparse_system_create) and does NOT own the batch.
 *   set_values   values_host = double[N][16], column-major 4x4 (all orthonormal to 1e-9: the rigid kernels serve the graph from then on; else the general ones).  Whatever
 *                the values, the relative pose of a factor is inverse(T_target) T_source with inverse(R, t) = (R^T, -R^T t): non-orthonormal values are inverted by
 *                transpose, as gtsam::Pose3::inverse;  get_values: the current values (after accept: the accepted trial's, as the device computed them)
 *   linearize    asynchronous: the batch's linearise at the current values' relative poses -> records in HBM
 *   try_lambda   damped step + retract (Pose3::retract: T Expmap(xi), xi = (omega, v) = the step's six entries of the pose's slot) + the batch's error evaluation on the
 *                linearisation's correspondences at the trial values: queued back to back, ONE wait (a poll of the evaluation's completion words).  x_host [6 slots], b_host [6 slots], c_host (the cost at the
 *                linearisation point), new_error (the cost at the trial values), new_values_host [N][16]; any may be NULL.  GP_ERROR_INDETERMINATE: b / c valid, no trial.
 *   accept       the last successful trial's values become the current ones (a swap: their relative poses are already in place); linearize again before the next trial
 *   optimize     the reference's loop over the three: GTSAM's LevenbergMarquardtParams defaults in gp_lm_params_default; lambda I damping only (diagonalDamping = false) */
typedef struct gp_lm_graph gp_lm_graph_t;
typedef struct gp_lm_params {
  double lambda_initial, lambda_factor, lambda_upper_bound, lambda_lower_bound; /* 1e-5, 10, 1e5, 0 */
  double relative_error_tol, absolute_error_tol, min_model_fidelity;            /* 1e-5, 1e-5, 1e-3 */
  double min_diagonal, max_diagonal;                                            /* 1e-6, 1e32 (diagonal damping only) */
  int max_iterations, diagonal_damping;                                         /* 100, 0 */
} gp_lm_params;
typedef struct gp_lm_summary {
  int iterations, inner_iterations; /* linearisations, trials */
  int gave_up;                      /* lambda reached lambda_upper_bound */
  int reserved_;
  double final_error, final_lambda;
} gp_lm_summary;
void gp_lm_params_default(gp_lm_params* params);
int gp_lm_graph_create(gp_vgicp_batch_t* batch, const int* pose_pairs, int num_poses, const unsigned char* pose_fixed, int ordering, gp_lm_graph_t** out);
int gp_lm_graph_destroy(gp_lm_graph_t* graph);
int gp_lm_graph_num_variables(const gp_lm_graph_t* graph); /* 6 x free poses */
int gp_lm_graph_set_values(gp_lm_graph_t* graph, const double* values_host);
int gp_lm_graph_get_values(gp_lm_graph_t* graph, double* values_host);
int gp_lm_graph_linearize(gp_lm_graph_t* graph);
int gp_lm_graph_try_lambda(gp_lm_graph_t* graph, double lambda, int diagonal_damping, double min_diagonal, double max_diagonal, double* x_host, double* b_host, double* c_host,
                           double* new_error, double* new_values_host);
int gp_lm_graph_accept(gp_lm_graph_t* graph);
/* speculation (on by default): behind a trial's error evaluation the linearise at the TRIAL values is queued into a second record buffer, so that an accepted step finds
 * its linearisation already running while the host decides (a rejected one wastes that launch); 0 = off.  Same bits either way.  Returns the previous setting. */
int gp_lm_graph_set_speculation(gp_lm_graph_t* graph, int enable);
/* the graph's own damped system: gp_sparse_system_set_one_launch / gp_dense_system_set_one_launch passed through (0: the multi-launch step, the retract as a kernel of
 * its own behind it; default 1: the one-launch step where the system qualifies, the retract as its epilogue).  Same bits. */
int gp_lm_graph_set_one_launch(gp_lm_graph_t* graph, int enable);
int gp_lm_graph_optimize(gp_lm_graph_t* graph, const gp_lm_params* params, gp_lm_summary* summary);
/* for checkers: the records of the last linearise (the VGICP batch's F, then the corr batch's G: gp_lm_graph_create_with_factors, then the pose factors' P:
 * gp_lm_graph_create_with_pose_factors) and the relative poses of the current values (the VGICP members'), where
 * they lie in device memory (valid until the graph is destroyed; contents as of the work queued so far on the graph's stream) */
int gp_lm_graph_records(gp_lm_graph_t* graph, const gp_linearized6** records_dev, const double** relative_poses_dev);

/* ---- gtsam::BetweenFactor<Pose3> / gtsam::PriorFactor<Pose3> with a Gaussian noise model (gp_pose_factors.hip) ----
 * GTSAM 4.2, default build (GTSAM_POSE3_EXPMAP on, GTSAM_SLOW_BUT_CORRECT_BETWEENFACTOR off); poses column-major 4x4, tangent order (omega, v), Lambda = R^T R of the
 * noise model in that order:
 *   between (pose_a, pose_b, measured Z):  e = Logmap(Z^-1 T_a^-1 T_b), J_a = -AdjointMap((T_a^-1 T_b)^-1), J_b = I (no LogmapDerivative(e): GTSAM's own choice)
 *   prior (pose_a, Z; pose_b = -1):        e = Logmap(Z^-1 T_a), J_a = I
 * Each factor linearises into ONE gp_linearized6 record: error = 1/2 e^T Lambda e (the factor's error(), as a VGICP record's error is that factor's error(); a caller
 * that builds a gtsam::HessianFactor from a record passes f = 2 error), num_inliers = 0; between: target = pose_a, source = pose_b (a VGICP factor is evaluated at
 * target^-1 source), H_target = J_a^T Lambda J_a, H_source = Lambda, H_target_source = J_a^T Lambda, b_target = J_a^T Lambda e, b_source = Lambda e; prior: a unary
 * record (H_source = Lambda, b_source = Lambda e, the rest 0) whose target slot is negative in gp_*_system_create's factor_slots.
 * create refuses (GP_ERROR_INVALID_ARGUMENT, before any device work): a pose out of [0, num_poses), a between factor with pose_a = pose_b, a prior with pose_b != -1,
 * an unknown kind, a measured pose that is not orthonormal to 1e-9 with det > 0, an information matrix that is not finite or not symmetric to 1e-12 x its largest entry.
 * The _dev forms are asynchronous on the stream given to create (poses_dev = double[num_poses][16]); the others copy the poses up, wait and copy the results down. */
#define GP_POSE_FACTOR_BETWEEN 0
#define GP_POSE_FACTOR_PRIOR 1
typedef struct gp_pose_factor {
  int kind, pose_a, pose_b, reserved_; /* prior: pose_b = -1 */
  double measured[16];                 /* column-major 4x4, orthonormal to 1e-9 */
  double information[36];              /* Lambda, (omega, v) order, column-major, symmetric, finite */
} gp_pose_factor;                      /* 432 B */
typedef struct gp_pose_factors gp_pose_factors_t;
int gp_pose_factors_create(const gp_pose_factor* factors, int num_factors, int num_poses, gp_stream_t stream, gp_pose_factors_t** out);
int gp_pose_factors_destroy(gp_pose_factors_t* pf);
int gp_pose_factors_size(const gp_pose_factors_t* pf); /* num_factors; 0 for NULL */
int gp_pose_factors_issue_linearize_dev(gp_pose_factors_t* pf, const double* poses_dev, gp_linearized6* out_dev); /* out_dev [num_factors] */
int gp_pose_factors_issue_compute_error_dev(gp_pose_factors_t* pf, const double* poses_dev, double* out_dev);      /* out_dev [num_factors] */
int gp_pose_factors_linearize(gp_pose_factors_t* pf, const double* poses_host, gp_linearized6* out_host);
int gp_pose_factors_compute_error(gp_pose_factors_t* pf, const double* poses_host, double* out_host);
/* an LM graph of VGICP factors (batch, pose_pairs as gp_lm_graph_create; batch may be NULL: a pure pose graph) and num_pose_factors pose factors over the same
 * num_poses poses.  Records: the batch's at [0, F), the pose factors' at [F, F + num_pose_factors) in the caller's order (gp_lm_graph_records); the damped system
 * covers all of them, c and new_error are the graph's error() (new_error: the VGICP errors in factor order, then the pose factors' in order, one host sum).
 * try_lambda evaluates the pose factors at the trial values behind the retract (errors -- and, speculating, the records at the trial values -- in ONE launch) and keeps
 * its one wait.  pose_fixed may be NULL (priors fix the gauge); stream: the graph's stream when batch is NULL, else NULL or the batch's own.  set_values of such a graph
 * refuses values that are not orthonormal to 1e-9 (GP_ERROR_INVALID_ARGUMENT).  Refusals as gp_pose_factors_create, and a graph with no factor at all. */
int gp_lm_graph_create_with_pose_factors(gp_vgicp_batch_t* batch, const int* pose_pairs, const gp_pose_factor* pose_factors, int num_pose_factors, int num_poses,
                                         const unsigned char* pose_fixed, int ordering, gp_stream_t stream, gp_lm_graph_t** out);
/* ... and with a batch of GICP / ICP factors (gp_corr_batch_*) as a third group: corr member i is the pairwise factor between poses corr_pairs[2 i] (target) and
 * corr_pairs[2 i + 1] (source), evaluated at target^-1 source like a VGICP member.  Any of the three groups may be absent (batch NULL, corr NULL, num_pose_factors 0),
 * not all of them.  Records (gp_lm_graph_records), and the order of the host's sum for new_error: the VGICP batch's at [0, F), the corr batch's at [F, F + G), the
 * pose factors' at [F + G, F + G + P); the damped system covers all of them.  The graph borrows both batches; they share one stream (`stream`: NULL or that stream
 * when a batch is given).
 * Sets and speculation: linearize searches the corr members' correspondences into the set that goes with the current record buffer; try_lambda evaluates their errors
 * on THAT set at the trial values (queued in front of the VGICP batch's evaluation, whose completion words then cover it; without a VGICP batch the corr batch's own
 * words are polled: one wait either way); the speculative linearise at the trial values searches into the OTHER set, and accept swaps set and record buffer together.
 * A rejected trial therefore leaves the correspondences of the linearisation point in place for the next lambda.  The graph's rigid flag (set_values) is passed on. */
int gp_lm_graph_create_with_factors(gp_vgicp_batch_t* batch, const int* vgicp_pairs, gp_corr_batch_t* corr, const int* corr_pairs, const gp_pose_factor* pose_factors,
                                    int num_pose_factors, int num_poses, const unsigned char* pose_fixed, int ordering, gp_stream_t stream, gp_lm_graph_t** out);

/* ---- PlaneEVMFactor / EdgeEVMFactor: BALM bundle adjustment by eigenvalue minimisation (gp_ba_factors.hip) ----
 * factors/bundle_adjustment_factor_evm.hpp, balm_feature.hpp, src/gtsam_points/factors/bundle_adjustment_factor_evm.cpp (Liu & Zhang, BALM, RA-L 2021).  One factor
 * is one feature seen from K poses with N points; with q_i = T_pose(i) p_i its error is error_scale lambda_0 of cov(q) (plane) or lambda_0 + lambda_1 (edge: the
 * reference's EdgeEVMFactor ignores error_scale in error() and linearize(), and so does this), its HessianFactor (keys, G = scale D^T H D, g = -scale J D, f = error)
 * with D_i = [-[q_i]x, I]: the derivative for a world-frame (left) perturbation, tangent order (omega, v), handed on unchanged as the reference does.  All f64.
 *   create        kinds [F] (GP_BA_PLANE / GP_BA_EDGE), error_scales [F], feature_offsets [F + 1] (feature f owns points [offsets[f], offsets[f + 1])), point_pose
 *                 [num_points] (the pose index of each point, any order within a feature: the host sorts a feature's points by pose), points double[num_points][3].
 *                 Everything is copied.  GP_ERROR_INVALID_ARGUMENT before any device work for: a NULL array or out, a count < 1, offsets that do not start at 0, are
 *                 not sorted or do not end at num_points, a feature with fewer than 3 points, a pose index outside [0, num_poses), an unknown kind.
 *   records       linearize writes R = U + Q gp_linearized6 records: first U unary records, one per pose that some feature touches, in pose order (target slot -1,
 *                 source = the pose, like a prior's record: H_source = sum over features of G_aa, b_source = -sum g_a), then Q pair records, one per pose pair a < b that
 *                 some feature co-observes, in (a, b) order (target a, source b, H_target_source = sum G_ab, the rest 0).  A feature's f and point count are the error /
 *                 num_inliers share of the unary record of its LOWEST pose, so the sum of `error` over the records is the total.  factor_slots: out int[R][2] =
 *                 (-1 | slot_of_pose[a], slot_of_pose[b]) for gp_dense_system_create / gp_sparse_system_create; a held pose (slot < 0) drops out as for every other
 *                 factor, the errors stay in c.
 *   bits          every sum has a fixed order and no atomics: two linearises at the same values agree bit for bit, and so do linearize and issue_linearize_dev.
 *   values        values_host / poses_dev = double[num_poses][16], column-major 4x4.  issue_linearize_dev is asynchronous on the stream given to create; the others
 *                 copy the values up, wait and copy the results down.  compute_errors: errors_host [F], each feature's error().
 *   feature_hessian  feature i's own dense factor over its K = feature_num_poses(i) poses in ascending pose order: G [6K][6K] (symmetric, full), g [6K], f --
 *                 through the same kernels, for single-factor callers and for checkers.
 * A repeated eigenvalue gives inf / NaN, as in the reference. */
#define GP_BA_PLANE 0
#define GP_BA_EDGE 1
typedef struct gp_ba_factors gp_ba_factors_t;
int gp_ba_factors_create(const int* kinds, const double* error_scales, const int* feature_offsets, const int* point_pose, const double* points, int num_features, int num_points,
                         int num_poses, gp_stream_t stream, gp_ba_factors_t** out);
int gp_ba_factors_destroy(gp_ba_factors_t* b);
int gp_ba_factors_num_records(const gp_ba_factors_t* b); /* R; 0 for NULL */
int gp_ba_factors_factor_slots(const gp_ba_factors_t* b, const int* slot_of_pose, int* out);
int gp_ba_factors_linearize(gp_ba_factors_t* b, const double* values_host, gp_linearized6* records_host);
int gp_ba_factors_issue_linearize_dev(gp_ba_factors_t* b, const double* poses_dev, gp_linearized6* records_dev);
int gp_ba_factors_compute_errors(gp_ba_factors_t* b, const double* values_host, double* errors_host);
int gp_ba_factors_feature_num_poses(const gp_ba_factors_t* b, int feature); /* K; 0 for NULL or a feature out of range */
int gp_ba_factors_feature_hessian(gp_ba_factors_t* b, int feature, const double* values_host, double* G, double* g, double* f);

/* ---- voxelgrid_sampling / randomgrid_sampling / sample on the device (gp_sampling.hip) ----
 * Device counterparts of types/point_cloud_cpu.hpp:110-156 (point_cloud_cpu_funcs.cpp:27-75, 119-295, 298-456; CPU-only upstream).
 * A plan is built once per (cloud, resolution); any number of attribute reductions or index selections then run on it, on the plan's stream.
 *   voxel      floor(double(p) * (1.0 / resolution)) per axis (:128,136).
 *   dropped    a point that is not finite, or whose coordinate + 2^20 falls outside [0, 2^21 - 1] on some axis (:132-140): counted in num_dropped, in NO output
 *              (the reference lumps such points under one invalid key and emits a NaN row for them; that row is not reproduced).
 *   order      voxels are numbered in ascending order of the reference's packed key (z << 42 | y << 21 | x of the offset coordinates, :143-146), i.e.
 *              lexicographically by (z, y, x) -- the order of the reference's single-threaded run; inside a voxel the points are in ascending point index.
 *   one row per voxel: the reference cuts its sorted array into blocks of 1024 and emits a voxel that straddles a cut once per block (:188-206), an artefact of
 *              its threading.  The device emits exactly one row per occupied voxel.
 * plan_create waits once (for num_voxels); num_points == 0 gives a valid empty plan without touching a device.
 * plan_average: out[v] = arithmetic mean of the rows of voxel v (Averager, :95-116) for any float attribute of width 1 .. 16 (points 3, covariances 9, normals 3 --
 *   not re-normalised, as upstream --, intensities 1, times 1): accumulated and divided in f64, rounded once to f32, no floating-point atomics; bit-identical from
 *   run to run and independent of which other attributes are reduced.  attr_dev float[num_points][width], out_dev float[num_voxels][width].  Asynchronous.
 * plan_random_indices (randomgrid_sampling): points_per_voxel = ceil(sampling_rate * N / num_voxels) (:377) with N = the valid points and num_voxels = the occupied
 *   voxels (the reference counts the key CHANGES of its sorted array, one less than its groups, the invalid group included); a voxel with fewer points keeps all
 *   of them, every other voxel exactly points_per_voxel: those with the smallest counter-based hash of (seed, point index), ties by index.  No generator state: the
 *   same seed gives the same selection on every run (mt19937 parity is neither possible nor wanted).  If the total exceeds size_t(N * sampling_rate * 1.2)
 *   (:378,445-449) that many are kept, again the smallest hashes.  sampling_rate >= 0.99 selects every valid point (:300-303).  The indices are written in ascending
 *   order (:451-452) to indices_out_dev (capacity num_points); *num_selected is valid on return (the call waits).
 * gp_cloud_gather: out[i] = attr[indices[i]] for float rows of `width` -- sample() (:27-75); the indices must lie inside attr (not checked).  Asynchronous.
 * GP_ERROR_INVALID_ARGUMENT before any device work: NULL arrays, a resolution that is not positive and finite, width outside 1 .. 16, a sampling rate outside (0, 1]. */
typedef struct gp_voxelgrid_plan gp_voxelgrid_plan_t;
int gp_voxelgrid_plan_create(const float* points_dev, int num_points, double resolution, gp_stream_t stream, gp_voxelgrid_plan_t** out);
int gp_voxelgrid_plan_info(const gp_voxelgrid_plan_t* plan, int* num_voxels, int* num_dropped);
int gp_voxelgrid_plan_average(gp_voxelgrid_plan_t* plan, const float* attr_dev, int width, float* out_dev);
int gp_voxelgrid_plan_random_indices(gp_voxelgrid_plan_t* plan, double sampling_rate, unsigned long long seed, int* indices_out_dev, int* num_selected);
int gp_voxelgrid_plan_destroy(gp_voxelgrid_plan_t* plan);
int gp_cloud_gather(const float* attr_dev, int width, const int* indices_dev, int num_indices, float* out_dev, gp_stream_t stream);
/* test hooks (thread-local, no device state): force_wide_keys != 0 makes every plan of this thread take the two-sort route (the one a bounding box of more than
 * 2^32 - 1 cells takes); the next `sort_faults` plan builds / index selections / time sorts (gp_cloud_sort_by_time_indices) see their first sort report an expired wait and must run again through the one-class
 * sort.  Returns how many did so far.  gp_debug_sample_hash: the rank value of (seed, point index), host code. */
int gp_debug_voxelgrid_hooks(int force_wide_keys, int sort_faults);
unsigned gp_debug_sample_hash(unsigned long long seed, unsigned index);

/* ---- remove_outliers / filter / sort_by_time on the device: index selections for gp_cloud_gather (gp_knn.hip, gp_cloud_filter.hip) ----
 * Device counterparts of find_inlier_points / remove_outliers (point_cloud_cpu_funcs.cpp:576-650), filter / filter_by_index (point_cloud_cpu.hpp:158-203) and
 * sort_by_time (point_cloud_cpu_funcs.cpp:459-465); CPU-only upstream.  Each produces int indices; sample() = gp_cloud_gather carries the attributes.
 * mean_neighbor_distances: d_i = (sum_{j < k} |p_nbr(i,j) - p_i|) / k over the k nearest points of the cloud itself (the point is its own first neighbour, distance
 *   0), 1 <= k <= 32, on a gp_point_grid built over these same points.  One fused kernel: the search's list stays in registers, the k square roots are added in list
 *   order (ascending distance, so the sum does not depend on which of several equidistant neighbours the search kept) in f64, one double per point is stored; no
 *   [n][k] array exists on this path.  SHORT points -- a non-finite coordinate, or fewer than k neighbours (n < k) -- store +inf and are counted in *num_short
 *   (host int, may be NULL; the call waits only when it is given).
 * mean_neighbor_distances_from: the same from the caller's lists neighbors_dev int[n][k], any k >= 1 (the second upstream overload); differences in f64 on the f32
 *   coordinates, written as the search writes them (the tests hold the two paths to the same bytes; by contract they agree to (k + 8) 2^-52 d_i).  An index outside [0, n) makes the point short and is never dereferenced.
 * inlier_threshold: over the FINITE entries of mean_dists (m of them): mean = sum d / m, var = sum d^2 / m - mean^2 (one pass, not clamped, :598-600),
 *   thresh = mean + sqrt(var) * std_thresh; stats_host double[4] = {mean, var, thresh, m}; m = 0 gives all zeros.  Sums in f64 in an order fixed by n alone
 *   (per-workgroup partials in workgroup order, lanes in a shuffle tree): two runs are bit-identical.  Waits.
 * select_below: the i with values[i] < thresh (strict) and values[i] finite; select_mask: the i with mask[i] != 0.  Both write ascending indices to
 *   indices_out_dev (capacity n) and wait: *num_selected is valid on return.
 * sort_by_time_indices: the permutation that sorts times ascending, stable (equal times in ascending index -- one of std::sort's legal outcomes); -0.0 = +0.0,
 *   NaN times last in ascending index.  indices_out_dev int[n].  Waits (for the radix sort's fault words; a faulted sort runs again in its one-class form).
 * GP_ERROR_INVALID_ARGUMENT before any device work: NULL arrays with n > 0, n < 0, k outside its range, a std_thresh that is not finite.  n == 0 is legal
 * everywhere: nothing is launched, nothing selected. */
int gp_cloud_mean_neighbor_distances(const gp_point_grid_t* grid, const float* points_dev, int n, int k, double* mean_dists_dev, int* num_short, gp_stream_t stream);
int gp_cloud_mean_neighbor_distances_from(const float* points_dev, int n, const int* neighbors_dev, int k, double* mean_dists_dev, int* num_short, gp_stream_t stream);
int gp_cloud_inlier_threshold(const double* mean_dists_dev, int n, double std_thresh, double* stats_host, gp_stream_t stream);
int gp_cloud_select_below(const double* values_dev, int n, double thresh, int* indices_out_dev, int* num_selected, gp_stream_t stream);
int gp_cloud_select_mask(const unsigned char* mask_dev, int n, int* indices_out_dev, int* num_selected, gp_stream_t stream);
int gp_cloud_sort_by_time_indices(const float* times_dev, int n, int* indices_out_dev, gp_stream_t stream);

/* the symbolic phase alone (pure host code, no device needed): elimination order perm[k] = slot eliminated k-th, elimination tree
 * parent[k] (-1 = root), block counts and the schedule; any output pointer may be NULL */
int gp_sparse_symbolic(int num_slots, const int* factor_slots, int num_factors, int ordering, int* perm_out, int* parent_out, int64_t* nnz_a_blocks, int64_t* nnz_l_blocks,
                       int* num_subtrees, int* top_columns);
/* the schedule of the numeric phase (pure host code): launch levels (level 0 = the independent subtrees, then the chains of separator columns level by
 * level, one workgroup per chain), the critical path in columns (sum over the levels of the longest work list) and the number of work lists */
int gp_sparse_symbolic_schedule(int num_slots, const int* factor_slots, int num_factors, int ordering, int* num_levels, int* critical_columns, int* num_lists);
/* ... and its work lists one by one (pure host code; arrays of `capacity` >= num_lists ints): the level a list runs in, its columns, the 6x6 block products its columns
 * gather in all and the most a single column gathers */
int gp_debug_sparse_work_lists(int num_slots, const int* factor_slots, int num_factors, int ordering, int capacity, int* level, int* columns, int* products, int* max_column_products);

/* ---- per-handle tuning (not part of the reference API) --------------------------------------------------------------------------
 * Every knob below belongs to ONE batch / factor / map / search structure; the library keeps no process-global switches, so two
 * handles driven from two threads never see each other's settings (thread-compatible per handle, re-entrant across
 * handles; tests/test_vgicp_gpu.py::test_two_threads_two_batches).  The library reads NO environment variable (no getenv in csrc/): nothing that is
 * computed, launched or printed depends on the environment (the A/B variables of rounds 2-3 and GP_KNN_DEBUG are gone; tests/test_capi_cpu.py greps for it).
 *
 * GP_TUNE_KERNEL selects the tile-kernel family of a VGICP batch.  M = (C_B + R C_A R^T)^-1, the transform and the residual are f64
 * in every family; "f32 outer products" computes what follows the inverse in f32 (measured parity vs the CPU factor <= 1e-7
 * relative, gate 1e-5).  A family that does not apply to a batch falls back (GP_TUNE_EFFECTIVE_KERNEL reads what a built table runs):
 *   GP_KERNEL_REFERENCE  reference-shaped kernel (reference bucket table, 92 explicit sums for non-orthonormal poses): cross-check
 *   GP_KERNEL_HASHED     pipeline kernel over the hashed line table, f32 outer products: maps without a block grid
 *   GP_KERNEL_GRID_F64   pipeline kernel over the occupancy-block grid, f64 throughout
 *   GP_KERNEL_LOOKAHEAD  round-2 pipeline kernel (block grid, f32 outer products, look-ahead lookup): maps with >= 2^26 voxels
 *   GP_KERNEL_STREAM     third generation (csrc/gp_vgicp_stream.hpp): per-wave chunk streams, balanced single-factor launches,
 *                        surface validation inside the ring.  Default.
 * (The A/B switches of rounds 2-3 -- poses by copy engine, finalize parts / width / host expansion, the fused GICP kernel -- were measured, decided and removed:
 *  profiles/r02_*, r03_*, DESIGN.md.) */
#define GP_FAR_POSE_RATIO_DEFAULT 2
enum {
  GP_KERNEL_REFERENCE = 0,
  GP_KERNEL_HASHED = 2,
  GP_KERNEL_GRID_F64 = 3,
  GP_KERNEL_LOOKAHEAD = 8,
  GP_KERNEL_STREAM = 12
};
enum {
  GP_TUNE_KERNEL = 0,           /* GP_KERNEL_* */
  GP_TUNE_SOURCE_POLICY = 1,    /* cache policy of the source stream: 0 per batch (non-temporal iff no two factors share a source cloud), 1 default, 2 non-temporal */
  GP_TUNE_XCD_CHUNK = 2,        /* workgroup -> tile map: 0 = every XCD walks a contiguous eighth of the tile list, c > 0 = runs of c tiles dealt round robin */
  GP_TUNE_STAGGER = 3,          /* round-2 kernels: the odd wave slots of every SIMD start `value` x 512 clocks late (0 = off) */
  GP_TUNE_TILE_INTERLEAVE = 4,  /* 1 = consecutive factors that share a source cloud take turns tile by tile, 0 (default) = factor-major */
  GP_TUNE_BALANCE = 5,          /* stream kernel, one large factor: how much more a dispatch round of workgroups takes than the next one, in 1/1000 of
                                   the mean share (0 = flat split .. 1000; -1 = automatic, the default: 150; a skew that would leave an XCD's last round less than a third
                                   of the mean share is dealt flat; a compute unit issues from its oldest waves first, csrc/gp_vgicp_shared.hpp) */
  GP_TUNE_EFFECTIVE_KERNEL = 6, /* read-only: the family the batch's current table runs (-1 before the first pass) */
  GP_TUNE_XCD_WEIGHT_0 = 8,     /* .. + 7: stream kernel, one large factor: share of XCD x in 1/1000 of the mean share (500..1500); setting any of the eight
                                   replaces the library's measured table (the others then count as 1000) */
  GP_TUNE_FUSED_FINALIZE = 17,  /* synchronous rigid-pose linearise / error evaluation of the stream family: 1 (default) = ONE launch -- a large single factor: the tile
                                   workgroup whose arrival completes an eighth of the row list sums that eighth and hands the sums to the host; a batch or a small
                                   factor: the workgroup that stores a factor's last row sums, expands and delivers the factor's record.  0 = tile kernel, then finalize
                                   kernel.  The records of the two forms are bit-identical (the same functions in the same order, csrc/gp_vgicp_finalize.hpp).
                                   1.5-1.8 us off a 1 M-point step, 10-20 % off a 256- / 512-factor call (profiles/r03_fused_finalize.jsonl, r03_fused_by_factor.txt) */
  GP_TUNE_TILE_CHUNKS = 18,     /* stream family, fixed-tile launches (batches, small single factors): 64-point chunks per wave of a tile (a tile = 256 x value points);
                                   0 (default) = 8 when the batch has >= 2048 tiles of 2048 points, else the largest of 4 / 2 / 1 that still gives >= 768 tiles */
  GP_TUNE_TEST_ARRIVAL_SKEW = 20, /* test hook (batches only): puts the host's count of arrival counter 0 `value` ahead of the device's, as a lost launch would; the next fused
                                   step must notice that its completion words do not arrive, reset the counters and finish through the finalize kernel */
  GP_TUNE_MAX_WORKGROUPS = 19,  /* stream family, one large factor: workgroups of the planned launch, 8 .. 1024 (default 1024 = one resident round) */
  GP_TUNE_SOURCE_MIRROR = 21,   /* stream family: 1 (default) = the kernels stream the sources' packed private mirrors (36 B per point: 12 B point + the six floats of the
                                   symmetric covariance, chunk-major; built once per cloud at the first table build, shared by all factors on the cloud, only from
                                   covariances that are symmetric to the last bit -- records are bit-identical to 0 = the caller's arrays (12 + 36 B per point) */
  GP_TUNE_EFFECTIVE_MIRROR = 22,/* read-only: 1 when the batch's current table streams the packed mirrors (-1 before the first pass) */
  /* 23 was GP_TUNE_EXPERIMENT (measurement builds of the stream kernel for an A/B of round 5, removed with them): the key is not reused, setting it fails with
     GP_ERROR_INVALID_ARGUMENT like any unknown key */
  GP_TUNE_TIMING = 7,           /* measurement: 1 = gp_vgicp_batch_linearize brackets its two kernels with HIP events (gp_vgicp_batch_last_kernel_ms) */
  GP_TUNE_MAP_BUILD = 16,       /* gp_voxelmap: 1 = reference-shaped hashed build (atomicCAS claims + atomic sums; also the fallback of clouds whose
                                   bounding box is too large for the block grid), 0 = binned deterministic build (default) */
  GP_TUNE_FAR_POSE_RATIO = 25,  /* VGICP factors / batches: a rigid pose whose translation exceeds `value` x the source cloud's extent (largest |coordinate|) takes the explicit-J_s
                                   sums instead of the 29 f32 sums + adjoint expansion (gp_vgicp_batch_takes_rigid_path); 0 = no pose counts as far (measurement: the rigid
                                   sums at any distance).  Default GP_FAR_POSE_RATIO_DEFAULT: half the largest ratio at which the rigid sums were measured inside 1e-6 of
                                   the f64 reference */
  GP_TUNE_BUCKET_LOAD = 24,     /* gp_voxelmap (binned build): load factor in per cent (5 .. 90, default 33) at which the reference-visible bucket table enters the reference's doubling
                                   sequence (gaussian_voxelmap_gpu.cu:269-291).  At 50 .. 67 % some probe chain among 10^5 voxels exceeds max_bucket_scan_count almost surely and the failed
                                   attempt costs a fill + an insertion pass + a wait; 33 % means up to twice the entries (16 B each) of a table sized at 67 % */
  GP_TUNE_KNN_STRUCTURE = 32    /* search structures (gp_point_grid, gp_estimate_covariances_ex, gp_gicp_factor): 0 = binned structure, per-lane search
                                   (default); 1 = hashed multi-level grid (also the fallback of clouds whose bounding box is too large for the block
                                   grid); 3 = as 0 with the row-tiled covariance pass in front of the per-lane search (exact, measured slower:
                                   DESIGN.md section 4.8); 4 = as 0 with a second binned level between the cells and the superblocks; 6 = as 0 with the covariance queries in plain
                                   cell-sorted order (round 3) instead of heavy-first (own-cell population < k first: round 4), for the A/B; 7 = as 0 without round 5's
                                   cooperative pass (covariance_far_kernel: sparse neighbourhoods searched by one wave per query), i.e. round 4's search, for the A/B; >= 16: staging experiment of round 4,
                                   16 | fine shells << 4 | shells of blocks << 8 (measured: no effect, profiles/r04_c5_staging.jsonl) */
};
int gp_vgicp_batch_set_tuning(gp_vgicp_batch_t* batch, int key, int value);
int gp_vgicp_batch_get_tuning(const gp_vgicp_batch_t* batch, int key, int* value);
/* with GP_TUNE_TIMING = 1: the durations of the tile kernel and of the finalize kernel of the last synchronous gp_vgicp_batch_linearize[_view],
 * i.e. of the kernels as they run INSIDE a step (behind the idle queue the host leaves between two passes), HIP events on the batch's stream */
int gp_vgicp_batch_last_kernel_ms(const gp_vgicp_batch_t* batch, float* tile_ms, float* finalize_ms);
/* fused synchronous single-factor linearise steps (GP_TUNE_FUSED_FINALIZE = 1) time themselves on the device's 100 MHz constant clock: the first workgroup of
 * every XCD stores its start, every part's finalizer when the part's last partial row was in and when its sums left for the host.  Since the last reset:
 * number of such steps, mean duration of the streaming part (first start .. last row in: what the roofline fraction is quoted on, as the step ran it) and
 * of the whole kernel's work (.. last sums out), in microseconds.  No events, no profiler, nothing added to the step but three 8-byte stores per part. */
int gp_vgicp_batch_device_times(gp_vgicp_batch_t* batch, int reset, double* steps, double* stream_us_mean, double* kernel_us_mean);
/* the per-factor entry points (gp_vgicp_factor_linearize, ..._issue_*) run a batch of one: this is its tuning */
int gp_vgicp_factor_set_tuning(gp_vgicp_factor_t* factor, int key, int value);
int gp_voxelmap_set_tuning(gp_voxelmap_t* map, int key, int value);
/* host-side check hook (runs without a device): the 29 target-side sums of a rigid pass (ACC layout of csrc/gp_device.hpp: count, error,
 * M[6], K[9], TL[6], q x Mr [3], Mr [3]) and the pose delta (column-major 4x4) -> the complete record, i.e. H_t from the sums and
 * H_s = Ad^T H_t Ad, H_ts = -H_t Ad, b_s = -Ad^T b_t (integrated_vgicp_factor_gpu.cpp:199-213 consumes them).  This is the expansion the
 * synchronous single-factor call runs on the host on the added sums of its finalize parts. */
int gp_debug_expand_rigid(const double sums[32], const double pose[16], gp_linearized6* out);
/* host-side check hook (runs without a device): the tiles (first point, number of points) a planned single-factor launch of the stream kernel deals
 * to its workgroups for a factor of n points and a GP_TUNE_BALANCE value, in tile-list order (XCD-major); *num_tiles = workgroups of the launch */
int gp_debug_stream_plan(int n, int skew_permille, const int* xcd_weights_permille /* [8] or NULL = the library's table */, int capacity, int* begin, int* count,
                         int* num_tiles);
/* ... and with the launch's other inputs, down to the waves: tile_points == 0 = the planned launch of at most max_workgroups (8 .. 1024, GP_TUNE_MAX_WORKGROUPS) workgroups;
 * tile_points > 0 (a multiple of 256) = the fixed tiles of a factor below the planning threshold, in tile order.  waves (or NULL): [capacity * 4][3] = first point, full
 * 64-point chunks and tail points of each of the four waves of every workgroup, as the stream kernel splits them */
int gp_debug_stream_plan_ex(int n, int tile_points, int max_workgroups, int skew_permille, const int* xcd_weights_permille /* [8] or NULL */, int capacity, int* begin,
                            int* count, long long* waves, int* num_tiles);
/* host-side check hook (runs without a device): for an explicit shard assignment, *rows_per_shard = rows every rank contributes to the in-place ncclAllGather of a
 * multi-device pass (0: the plan does not allow it -- unequal or non-contiguous shards -- and the pass all-reduces), and send_offset_doubles[k] = where shard k's send
 * buffer starts inside the [F x width] stack, in doubles.  Runs the functions gp_vgicp_multi_batch_* itself uses. */
int gp_debug_multi_gather_plan(const int* shard_of_factor, int num_factors, int num_shards, int width, int64_t* rows_per_shard, int64_t* send_offset_doubles);
/* gp_estimate_covariances runs its second launch on a low-priority side stream; two streams overlap only when their hardware queues sit on different dispatch pipes, so
 * the library probes (once per host thread and device, beside the first caller stream) up to four candidate streams and keeps the one whose queue does not wait for the caller's grid
 * (gp_side_stream.hip, SideStream).  This returns the measured delays in microseconds (< 0 = not probed) and the index of the stream in use beside `caller`. */
int gp_debug_side_stream_probe(gp_stream_t caller, float delays_us[4], int* chosen);
/* test hooks for the structure builds' sort fallback (gp_sort.hpp / gp_binning.hip; thread-local, no device state): the next `count` builds of this thread (voxel-map
 * insert, k-NN structure) see their first radix sort report "a tile waited for a workgroup that was never started" and must rebuild through the one-class sort;
 * count < 0: the next |count| builds, and the faulted sort also leaves garbage keys (far outside every cell range) in part of its output, as a really expired wait does.
 * gp_debug_sort_fallbacks = how many builds of this thread did so far. */
int gp_debug_inject_sort_fault(int count);
int gp_debug_sort_fallbacks(void);
/* test hook: the next `count` fused error evaluations of this batch (gp_vgicp_batch_compute_error, gp_vgicp_batch_compute_error_dev_end) read as if their
 * completion words had not arrived and take the recovery path.  Host side only: the kernels run as always.  0 disarms. */
int gp_debug_drop_error_words(gp_vgicp_batch_t* batch, int count);
/* timeline hook (measurement): per-workgroup phase timestamps (s_memtime) of THIS batch's single-factor linearise into dev_buffer
 * ([2048][16] uint64: slots 0-7 phases, 8 HW_ID, 9 XCC_ID, 10 / 11 start / end on the device-wide clock; row 2047: the finalize kernel of the
 * synchronous call); NULL disables */
int gp_vgicp_batch_set_trace_buffer(gp_vgicp_batch_t* batch, void* dev_buffer);

/* ---- global registration: FastOccupancyGrid, feature matching, RANSAC, closed-form alignment (csrc/gp_occupancy.hip, csrc/gp_feature_match.hip, csrc/gp_registration.hip) ----
 * Device counterparts of ann/fast_occupancy_grid.hpp, registration/ransac.hpp + impl/ransac_impl.hpp and registration/alignment.hpp; CPU-only upstream.  f64
 * arithmetic on the f32 device points throughout.
 *
 * gp_occupancy_grid: the SET of occupied cells of FastOccupancyGrid.  cell = fast_floor((pose * p) * (1 / resolution)) + 2^20 per axis, blocks of 8 x 8 x 8 cells,
 *   block key = three block coordinates masked to 21 bits in a uint64; coordinates outside 21 bits alias by the mask, as in the reference.  pose * p is evaluated
 *   as ((r0 x + r1 y) + r2 z) + t per row, each operation rounded once (no fused multiply-add).  A point whose transformed coordinates are not finite has no cell.
 *   The hash table is the library's own (64-bit compare-and-swap on keys, 32-bit OR on cell words; a power of two of slots, at most half full, sized from the
 *   number of points inserted; every probe loop is bounded by the table size) -- the reference's 10-probe limit and rehash are not reproduced: the set is exact.
 *   _insert: may be called any number of times, the result is the union; waits once (for the counts).  pose NULL = identity.
 *   _overlap: number of points of the cloud whose cell is in the set (calc_overlap); waits.  _get_overlaps: 0 / 1 per point into a device array; asynchronous.
 *   _overlap_batch: counts_out_dev[h] = calc_overlap(points, poses_dev[h]) for h < num_poses in ONE launch (poses_dev double[num_poses][16], column-major, on the
 *   device; counts int[num_poses] on the device); asynchronous.  This is RANSAC's scoring kernel. */
typedef struct gp_occupancy_grid gp_occupancy_grid_t;
int gp_occupancy_grid_create(double resolution, gp_stream_t stream, gp_occupancy_grid_t** out);
int gp_occupancy_grid_destroy(gp_occupancy_grid_t* grid);
int gp_occupancy_grid_insert(gp_occupancy_grid_t* grid, const float* points_dev, int num_points, const double* pose /* [16] or NULL */);
int gp_occupancy_grid_overlap(const gp_occupancy_grid_t* grid, const float* points_dev, int num_points, const double* pose /* [16] or NULL */, int* num_overlap);
int gp_occupancy_grid_overlap_batch(const gp_occupancy_grid_t* grid, const float* points_dev, int num_points, const double* poses_dev, int num_poses, int* counts_out_dev);
int gp_occupancy_grid_get_overlaps(const gp_occupancy_grid_t* grid, const float* points_dev, int num_points, const double* pose /* [16] or NULL */, unsigned char* overlaps_out_dev);
int gp_occupancy_grid_num_occupied_cells(const gp_occupancy_grid_t* grid);
/* (measurement) slots of the table and occupied blocks */
int gp_occupancy_grid_info(const gp_occupancy_grid_t* grid, int* num_slots, int* num_blocks);

/* Exact 1-NN among feature rows, brute force, tiled through LDS: for query i (row rows_dev[i] of query_features_dev, or row i when rows_dev is NULL)
 *   indices_out_dev[i] = argmin_t sum_j (q_j - target[t][j])^2, sq_dists_out_dev[i] = that minimum,
 * the differences and the sum in f64 on the f32 values (direct form, fused multiply-add accumulation in ascending j).  Features are float[N][dim] row-major on the
 * device, 1 <= dim <= 128 (GP_FEATURE_MAX_DIM).  Among targets at exactly the same f64 distance the LOWEST index is returned (the determinism of gp_ransac_estimate_pose rests on it).  A row index outside [0, num_query_rows),
 * or a query no target compares below +inf with (NaN features), gives index -1 and distance +inf.  Asynchronous on `stream`. */
#define GP_FEATURE_MAX_DIM 128
int gp_feature_nn_search(const float* target_features_dev, int num_target, const float* query_features_dev, int num_query_rows, int dim, const int* rows_dev, int num_queries,
                         int* indices_out_dev, double* sq_dists_out_dev, gp_stream_t stream);

/* estimate_pose_ransac (impl/ransac_impl.hpp:24-191), one device thread per hypothesis, iterations 0 .. max_iterations - 1 in chunks of chunk_iterations in stream order.
 * Per iteration, in this order (the first that applies is the iteration's status):
 *   sampling     dof 6: 3, dof 4: 2 distinct source indices (:39-48).  The d-th draw of iteration `it` (d = 0, 1, ... counts every draw, redraws included) is
 *                  index = ((r >> 32) * num_source) >> 32,  r = mix(mix(seed + G * (it + 1)) + G * (d + 1)),  G = 0x9E3779B97F4A7C15,
 *                  mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31),
 *                all in uint64 arithmetic modulo 2^64 (gp_ransac_sample_index is this function on the host).  A draw equal to an index already held is drawn again;
 *                more than 64 redraws in one iteration: GP_RANSAC_SAMPLE_FAILED.  std::mt19937 parity is neither possible nor wanted.  With sample_indices_dev
 *                (int[max_iterations][3], the third unused for dof 4) the caller's indices are taken as they are (they must lie inside the source cloud).
 *   invalid feature  a sampled source row with every |f_j| <= 1e-3 (Eigen's isZero(1e-3), :57): GP_RANSAC_INVALID_FEATURE
 *   matching     gp_feature_nn_search of the sampled rows among the target features (:62); a query without a match takes target 0, as the reference does (:64)
 *   polygon      max over the sample's edges of |dt - ds| / max(dt, ds, 1e-6) (:73-88) > poly_error_thresh: GP_RANSAC_POLY_REJECTED
 *   alignment    align_points_se3 / align_points_4dof of the sample (alignment.cpp:11-65): R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T from the two leading singular pairs
 *                of H's 3x3 block (one-sided Jacobi), which equals U diag(1, 1, det(U) det(V)) V^T; dof 4: the rotation about z that maximises trace(R^T H) on the 2x2 block
 *   taboo        angle(taboo^-1 T) < taboo_thresh_rot and |t(taboo^-1 T)| < taboo_thresh_trans for one of up to 64 poses (:149-156): GP_RANSAC_TABOO
 *   score        inliers = gp_occupancy_grid_overlap_batch of the source at T over a grid of the target at inlier_voxel_resolution (:115-117): GP_RANSAC_SCORED
 * Selection is deterministic (the reference's depends on thread timing): behind each chunk a device flag is set when one of its scored hypotheses has
 * inliers > num_source * early_stop_inlier_rate (:163); every kernel of a later chunk reads the flag first and leaves, its iterations get GP_RANSAC_SKIPPED.
 * The result is the scored hypothesis with the most inliers, ties to the lowest iteration; inlier_rate = best_inliers / num_TARGET (:190, the reference's own
 * denominator).  Without a scored hypothesis: identity, best_iteration -1, inlier_rate 0.  Everything is queued on one stream behind one host wait.
 * Per-iteration arrays (gp_ransac_hypotheses, each pointer a device array or NULL): status int[H]; source / target indices int[H][3] (-1 where not drawn / not
 * matched); poses double[H][16] column-major (zeros before the alignment); inliers int[H] (-1 where not scored).
 * GP_ERROR_INVALID_ARGUMENT before any launch: fewer source points than samples, an empty target, dof outside {4, 6}, dim outside 1 .. 128, more than 64 taboo
 * poses, max_iterations or chunk_iterations < 1, a resolution that is not positive and finite. */
enum { GP_RANSAC_SCORED = 0, GP_RANSAC_SAMPLE_FAILED = 1, GP_RANSAC_INVALID_FEATURE = 2, GP_RANSAC_POLY_REJECTED = 3, GP_RANSAC_TABOO = 4, GP_RANSAC_SKIPPED = 5 };
#define GP_RANSAC_MAX_TABOO 64
#define GP_RANSAC_MAX_REDRAWS 64
typedef struct gp_ransac_params {
  int max_iterations;              /* 5000 */
  int dof;                         /* 6 (SE3) or 4 (XYZ + RZ) */
  int chunk_iterations;            /* 1024 */
  int num_taboo;                   /* 0 */
  double early_stop_inlier_rate;   /* 0.8 */
  double poly_error_thresh;        /* 0.5 */
  double inlier_voxel_resolution;  /* 1.0 */
  double taboo_thresh_rot;         /* 0.5 degrees in radians */
  double taboo_thresh_trans;       /* 0.25 */
  uint64_t seed;                   /* 5489 */
  const double* taboo_poses;       /* host double[num_taboo][16], column-major */
} gp_ransac_params;
typedef struct gp_ransac_hypotheses {
  int* status;
  int* source_indices;
  int* target_indices;
  double* poses;
  int* inliers;
} gp_ransac_hypotheses;
typedef struct gp_ransac_result {
  double T_target_source[16];
  double inlier_rate;
  int best_inliers;
  int best_iteration;
  int num_scored;
  int early_stopped;
} gp_ransac_result;
void gp_ransac_params_default(gp_ransac_params* params);
unsigned gp_ransac_sample_index(uint64_t seed, unsigned iteration, unsigned draw, unsigned num_source); /* host code */
int gp_ransac_estimate_pose(const float* target_points_dev, int num_target, const float* source_points_dev, int num_source, const float* target_features_dev,
                            const float* source_features_dev, int dim, const gp_ransac_params* params, const int* sample_indices_dev, const gp_ransac_hypotheses* hypotheses,
                            gp_ransac_result* result, gp_stream_t stream);
/* the weighted N-point overloads of align_points_se3 / align_points_4dof (alignment.cpp:67-139): points double[N][3] and weights double[N] on the device, the
 * weighted means and H summed in a fixed tree order (no floating-point atomics), the rotation as above; pose_out: host double[16], column-major.  Waits. */
int gp_align_points(const double* target_points_dev, const double* source_points_dev, const double* weights_dev, int num_points, int dof, double* pose_out, gp_stream_t stream);

/* ---- fast global registration: graduated non-convexity from feature matches (csrc/gp_gnc.hip) ----
 * Device counterpart of registration/graduated_non_convexity.hpp and impl/graduated_non_convexity_impl.hpp:27-198 (Zhou et al., "Fast Global Registration");
 * CPU-only upstream.  Every per-correspondence rule is the reference's; the random numbers are this library's (gp_ransac_sample_index) and deterministic for a
 * seed.  The reference's three tree arguments have no counterpart (its target_tree is unused there too); num_threads and verbose have no meaning here.
 *
 * 1. correspondences (impl:27-84)
 *   query side   the SMALLER cloud queries: num_source < num_target: the source rows are searched among the target's features; otherwise (equal sizes too) the
 *                target rows are searched among the source's and the pairs are swapped back (:75-80, result `swapped` = 1).  Pairs are always (target, source).
 *   subsample    a query cloud of n > max_init_samples rows queries K = max_init_samples of them, in ascending order.  THIS LIBRARY'S RULE (the reference shuffles
 *                with std::mt19937, :37; parity is neither possible nor wanted): stratified, without a sort or a compaction -- for 0 <= j < K
 *                  lo = floor(j n / K), hi = floor((j + 1) n / K)  (64-bit integers),  index_j = lo + gp_ransac_sample_index(seed, j, 0, hi - lo),
 *                exactly K distinct ascending indices.  query_indices_dev (int[num_query_indices], ascending, distinct, inside the query cloud: the CALLER's duty)
 *                replaces the rule and the limit.
 *   matching     one gp_feature_nn_search with the query indices as rows (its lowest-index tie rule holds); with reciprocal_check a second one the other way
 *                round, rows = the forward matches: a pair is kept only where the answer is the query index itself (:61-68).  A query without a match (a NaN row) has
 *                no pair.  GNC has no invalid-feature rule: all-zero rows match like any other.
 *   compaction   pairs without a match are removed, the order is kept (:82-84); one host wait for the count.
 * 2. tuple test (:91-131), only if tuple_check and count > 3 max_num_tuples.  Tuple i < max_num_tuples draws the correspondences
 *   gp_ransac_sample_index(seed, i, k, count), k = 0, 1, 2 (not necessarily distinct: the reference does not require it); each of the three edges is tested as
 *   ratio = |t_a - t_b| / |s_a - s_b| (norms and quotient plain f64); the tuple is rejected if a ratio < tuple_thresh or > 1 / tuple_thresh (a 0 / 0 ratio is NaN,
 *   both comparisons are false, the tuple counts as valid: the reference's behaviour).  The pairs of the valid tuples are sorted by source index and made unique by
 *   source index (:122-123); where the reference's unstable sort leaves the surviving target unspecified, the LOWEST target index survives.
 * 3. the loop (:133-198), ONE launch of one workgroup and one host wait.  mu starts as the diagonal of the bounding box of the target's points with three finite
 *   coordinates (f32 widened to f64, sqrt((dx dx + dy dy) + dz dz); 0 without such a point), T as the identity.  for i < max_iterations { inner_iterations
 *   alignments; mu /= div_factor; if (mu < max_corr_dist) break; } -- the schedule is computed by the kernel itself, in f64, by the same sequence of divisions
 *   (the reference spells the field innter_iterations, graduated_non_convexity.hpp:28).  One alignment, for every pair j:
 *     e = |t - T s|^2, T s as ((r0 x + r1 y) + r2 z) + t per row, e = (dx dx + dy dy) + dz dz, no fused multiply-add;  q = mu / (mu + e), w = q q.
 *     THE REFERENCE'S SHADOWED VARIABLE IS REPRODUCED: the inner-iteration variable j (:150) is shadowed by the correspondence index j (:158), so `i == 0 && j == 0`
 *     (:165) forces w = 1 only for correspondence 0, during outer iteration 0, in EVERY inner iteration of it.
 *     sum of w, w t, w s, of e, and the count of e < (2 max_corr_dist)^2; then H = sum w (t - mean_t)(s - mean_s)^T with w recomputed by the same expression; the
 *     sums are fixed-order trees in LDS (no floating-point atomics: the same input gives the same bits on every run); the pose by the closed forms of
 *     gp_align_points (dof 6 / 4).  inlier_rate = that count / N of the LAST alignment, that is, at the pose BEFORE it (:187).
 *   trace (gp_gnc_trace, each pointer a device array of max_iterations * inner_iterations entries, or NULL; filled up to num_alignments): mu, sum_weights,
 *   sum_errors, num_inliers and the pose AFTER the alignment (double[16] column-major) -- the reference's `verbose` output.
 *   No correspondences (the reference divides by zero): identity, inlier_rate 0, num_correspondences 0, num_alignments 0, final_mu 0; no launch, no error.
 * gp_feature_correspondences: stages 1 - 2; pairs_out_dev int[capacity][2] (target, source) on the device, capacity = the number of queries (num_query_indices,
 *   or min(n, max_init_samples) of the query cloud); *num_pairs on the host.  The point arrays are read by the tuple test only (NULL without tuple_check).  Waits.
 * gp_gnc_align_correspondences: stage 3 on the caller's pairs (an index outside its cloud is never read: the pair's points become NaN).  Waits once.
 * gp_gnc_estimate_pose: all three; pairs_out_dev (as above) and trace may be NULL.
 * GP_ERROR_INVALID_ARGUMENT before any device work: dof outside {4, 6}, dim outside 1 .. 128, an empty cloud, div_factor <= 1 (or NaN), max_corr_dist,
 * max_iterations or inner_iterations not positive, max_init_samples < 1, tuple_check with max_num_tuples < 1, NULL arrays. */
typedef struct gp_gnc_params {
  int max_init_samples;  /* 5000 */
  int reciprocal_check;  /* 1 */
  int tuple_check;       /* 0 */
  int max_num_tuples;    /* 1000 */
  double tuple_thresh;   /* 0.9 */
  double div_factor;     /* 1.4 */
  double max_corr_dist;  /* 0.25 */
  int inner_iterations;  /* 3 (the reference's innter_iterations) */
  int max_iterations;    /* 64 */
  int dof;               /* 6 (SE3) or 4 (XYZ + RZ) */
  int reserved_;
  uint64_t seed;         /* 5489 */
} gp_gnc_params;
typedef struct gp_gnc_trace {
  double* mu;
  double* sum_weights;
  double* sum_errors;
  int* num_inliers;
  double* poses;
} gp_gnc_trace;
typedef struct gp_gnc_result {
  double T_target_source[16];
  double inlier_rate;
  double final_mu;          /* mu behind the last division */
  int num_initial;          /* queries of stage 1 (0 from gp_gnc_align_correspondences) */
  int num_correspondences;  /* pairs the loop ran on */
  int num_alignments;
  int swapped;              /* 1: the target rows were the queries */
} gp_gnc_result;
void gp_gnc_params_default(gp_gnc_params* params);
int gp_feature_correspondences(const float* target_points_dev, int num_target, const float* source_points_dev, int num_source, const float* target_features_dev,
                               const float* source_features_dev, int dim, const gp_gnc_params* params, const int* query_indices_dev, int num_query_indices, int* pairs_out_dev,
                               int* num_pairs, int* num_initial, int* swapped, gp_stream_t stream);
int gp_gnc_align_correspondences(const float* target_points_dev, int num_target, const float* source_points_dev, int num_source, const int* pairs_dev, int num_pairs,
                                 const gp_gnc_params* params, const gp_gnc_trace* trace, gp_gnc_result* result, gp_stream_t stream);
int gp_gnc_estimate_pose(const float* target_points_dev, int num_target, const float* source_points_dev, int num_source, const float* target_features_dev,
                         const float* source_features_dev, int dim, const gp_gnc_params* params, const int* query_indices_dev, int num_query_indices, int* pairs_out_dev,
                         const gp_gnc_trace* trace, gp_gnc_result* result, gp_stream_t stream);

/* ---- FPFH descriptors over a fixed-radius search (csrc/gp_fpfh.hip) ----
 * Device counterpart of estimate_fpfh (features/fpfh_estimation.hpp:57-66, src/gtsam_points/features/fpfh_estimation.cpp:58-93, :196-307; Rusu et al., "Fast Point
 * Feature Histograms"); CPU-only upstream.  points_dev, normals_dev: float[n][3] (normals as gp_estimate_normals_* writes them); all arithmetic f64 from there on.
 *   neighbourhood  every j with d2 = (dx dx + dy dy) + dz dz < search_radius^2, strictly; j = i included.  A point with a non-finite coordinate is nobody's neighbour;
 *                  its own SPFH / FPFH rows are zero and its num_neighbors is 0.  That holds for +-inf as for NaN; a finite coordinate of any size (3e38) is an ordinary
 *                  point, its own only neighbour unless another lies within the radius.
 *   truncation    THE ONE DEVIATION from the reference, which keeps the first max_num_neighbors points in its kd-tree's traversal order: here the cell coordinate is
 *                  floor(coord / search_radius) in f64 (clamped to +-(2^20 - 3)), the 27 cells around the query are walked in ascending (dz, dy, dx) order, dx
 *                  fastest, the points of a cell in ascending index, and the walk stops after max_num_neighbors accepted points.  Both passes walk by this rule.  It
 *                  decides anything only where the cap binds.  *num_truncated_out (host, may be NULL): the points with num_neighbors == max_num_neighbors.
 *   SPFH of k      num_neighbors <= 1: zero.  Otherwise the three 11-bin integer histograms of compute_pair_features(p_k, n_k, p_j, n_j) over every neighbour j != k (by
 *                  index) -- with its d == 0 zero return, its swap on |angle1| < |angle2| and its zero return when v = (ndp x n1) / |ndp x n1| is not finite --,
 *                  bin = clamp(floor((f - fmin) / range * 11), 0, 10), fmin = (-pi, -1, -1), range = (2 pi, 2, 2) (a NaN feature: bin 0), times 100.0 / (num_neighbors - 1).
 *   FPFH of i      num_neighbors <= 1: zero.  Otherwise the sum over the neighbours with d2 != 0 of spfh[j] * (1.0 / d2), times 100.0 / (sum of its first 11 entries):
 *                  that one normaliser for all 33 entries, as in the reference.  A row whose first 11 entries sum to zero (only coincident copies around) is NaN, as in
 *                  the reference (0 * inf).  spfh[j] is always j's SPFH over j's own neighbourhood, whether j is requested or not.
 *   determinism    integer histograms; the f64 sums of the FPFH pass are lane-strided partials added in a fixed tree; no floating-point atomics: the same input gives
 *                  the same bits.  The sum order is not the reference's (its neighbour order), so rows agree to rounding, not to the bit.
 * indices_dev: int[num_indices] rows to compute (any order, repeats allowed, inside [0, n): the CALLER's duty), or NULL = all n in order.  Outputs, each a device
 * array or NULL: fpfh_out_dev double[M][33], fpfh_out_f32_dev float[M][33] (the f64 value rounded once), spfh_out_dev double[n][33], num_neighbors_out_dev int[n].
 * With both FPFH outputs NULL only the SPFH pass runs.  With both set, one call writes both: the f64 array as it would alone, the f32 array those values rounded once.
 * indices_dev == NULL means all n points whatever num_indices says (0 included): a caller with an empty request passes no FPFH output.
 * Waits for the stream before it returns.
 * GP_ERROR_INVALID_ARGUMENT before any device work: NULL params, points or normals; n < 1 (or >= 2^30); search_radius not finite or <= 0; max_num_neighbors < 1;
 * num_indices < 0; no output at all. */
#define GP_FPFH_DIM 33
typedef struct gp_fpfh_params {
  double search_radius;  /* 5.0 */
  int max_num_neighbors; /* 10000 */
} gp_fpfh_params;
void gp_fpfh_params_default(gp_fpfh_params* params);
int gp_estimate_fpfh(const float* points_dev, const float* normals_dev, int n, const gp_fpfh_params* params, const int* indices_dev, int num_indices, double* fpfh_out_dev,
                     float* fpfh_out_f32_dev, double* spfh_out_dev, int* num_neighbors_out_dev, int* num_truncated_out, gp_stream_t stream);
/* measurement (scripts/fpfh_time.py): enable != 0 makes this thread's later gp_estimate_fpfh calls time their phases with events; ms_out (double[3] or NULL) receives
 * the stream time of the grid build, the SPFH pass and the FPFH pass of the last timed call */
int gp_debug_fpfh_phase_times(int enable, double* ms_out);
#ifdef __cplusplus
}
#endif
#endif /* GTSAM_POINTS_HIP_H */
