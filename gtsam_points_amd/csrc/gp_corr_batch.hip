// gp_corr_batch.hip -- a batch of matching-cost factors on nearest-neighbour correspondences (GICP, point-to-point and point-to-plane ICP, LOAM edge / plane /
// combined: gp_corr_factors.hip; colored GICP: gp_colored_factors.hip) whose relative poses live in DEVICE memory: what gp_vgicp_batch_issue_linearize_dev / _issue_compute_error_dev are to the VGICP factor, and what the device-resident LM graph
// (gp_lm.hip) queues for these factors.
//
// A single factor's linearise is three launches and a wait with its pose in the kernel arguments (gp_{gicp,icp}_factor_linearize); F of them are 3 F launches and F
// waits, and every pose goes through the host.  Here the launch count does not depend on F:
//   linearise       one search launch (gp_knn.hip: nearest_correspond_batch_kernel -- search structure, cloud, cut-off and pose of each factor from tables in device
//                   memory), one tile launch per factor KIND present (the kernels are instantiated per term: GICP, ICP point, ICP plane, colored GICP), one finalize launch
//   error           the tile launches (MODE_ERR) on the STORED correspondences -- the reference's error() does not search (integrated_gicp_factor_impl.hpp:183-185) --
//                   and one finalize launch
// The per-point terms, the 1024-point tiles dealt to 256 lanes, the reduction of a tile's sums (gp_corr_factors.hpp) and the finalize kernels (gp_vgicp.hip, one
// workgroup per factor over the factor's contiguous rows) are the single-factor call's own, on the same operands in the same order: a batch record has the bits of
// the single-factor call at the same pose.  A tile never straddles two factors (the flat tile list is built once, at create).
//
// Correspondences are kept in TWO sets.  The LM graph queues a speculative linearise at a trial's values behind the trial's error evaluation; were there one set, a
// REJECTED trial would leave the next trial evaluating on the correspondences of the rejected point instead of those of the linearisation point.  A linearise names
// the set it searches into, an error evaluation the set it reads; the partial rows of the two passes are separate buffers.
//
// LOAM members.  Internally the batch is a list of PARTS: a GICP or ICP member is one part, a LOAM member its edge part, its plane part, or both in that order.  Tiles,
// rows, search descriptors and the finalize kernels' table are per part.  With a two-part member present the parts outnumber the members, and two small launches
// frame a pass: one hands every part its member's pose, one adds a member's part records (errors) in part order in f64 into the member's record -- the sum
// gp_loam_factor_linearize forms on the host, so the bits agree.  Without one, part p IS member p and neither launch exists: a batch of GICP / ICP members runs
// exactly the launches it ran before.  The LOAM parts add one search launch (K = 2 and 3 together, gp_knn.hip: nearest_k_correspond_batch_kernel), one tile launch
// per term kind present, and the validation launch when a member enables it; none of these counts depends on the number of members.
//
// Colored GICP members.  One part each, behind the LOAM parts in record order (so a batch of the older kinds keeps its order), but a 1-NN kind: their tiles lie in the
// 1-NN prefix of the tile list, in front of the LOAM tiles, and the one nearest_correspond_batch_kernel launch searches them.  What the term reads beyond CorrBatchDesc
// (both intensities, the target's normals and gradients, photometric_term_weight) is in a table of its own, ColoredBatchDesc; the tile kernel is the GICP / ICP one
// instantiated with that table.  They add one tile launch per pass and nothing else.  A member's photometric_term_weight and max_correspondence_distance are read when
// the batch is created (as a LOAM member's cut-offs are): a later gp_colored_gicp_factor_set_* does not reach an existing batch.
// Not thread-safe per handle, re-entrant across handles, like the rest of the library.
#include <type_traits>
#include <vector>

#include "gp_colored_term.hpp"

namespace gp {

// what the tile kernels read of factor t.factor (every kind's pointers in one record; a kind reads its own)
struct CorrBatchDesc {
  const float* points;          // [n][3] source
  const float* covs;            // [n][9] source (GICP)
  const float* target_points;   // [num_target][3]
  const float* target_covs;     // [num_target][9] (GICP)
  const float* target_normals;  // [num_target][3] (ICP point-to-plane)
  const int* corr[2];           // [n] the two correspondence sets
};

template <class TERM>
__device__ __forceinline__ TERM batch_term(const CorrBatchDesc& d) {
  if constexpr (std::is_same<TERM, GicpTerm>::value) {
    return GicpTerm{d.points, d.covs, d.target_points, d.target_covs};
  } else {
    return TERM{IcpDesc{d.points, d.target_points, d.target_normals}};
  }
}

// what the colored GICP tile kernels read of part t.factor: the single factor's own term as it stood when the batch was created (a table of its own beside
// CorrBatchDesc, which the GICP / ICP kernels keep as it is)
struct ColoredBatchDesc {
  ColoredGicpTerm term;
  const int* corr[2];  // [n] the two correspondence sets
};

template <class TERM>
__device__ __forceinline__ TERM batch_term(const ColoredBatchDesc& d) {
  static_assert(std::is_same<TERM, ColoredGicpTerm>::value, "ColoredBatchDesc serves the colored GICP term only");
  return d.term;
}

// what the LOAM tile kernels and the validation read of part t.factor (a table of its own beside CorrBatchDesc, which the GICP / ICP kernels keep as it is)
struct LoamBatchDesc {
  const float* points;         // [n][3] source
  const float* target_points;  // [num_target][3]
  int* corr[2];                // int[K][n] each: the two correspondence sets
  int n;
  int k;         // 2: edge part, 3: plane part
  int validate;  // the member's enable_correspondence_validation
  int pad_;
};

template <class TERM>
__device__ __forceinline__ TERM batch_term(const LoamBatchDesc& d) {
  static_assert(TERM::kNeighbours > 1, "LoamBatchDesc serves the LOAM terms only");
  return TERM{LoamDesc{d.points, d.target_points}};
}

// corr_tile_kernel (gp_corr_tile.hpp) with the tile, the factor and the poses looked up: workgroup b takes tile tiles[b], lane t of 256 its points t, t + 256, ...
// DESC: CorrBatchDesc (GICP, ICP), ColoredBatchDesc (colored GICP) or LoamBatchDesc (LOAM edge, plane: a term is handed corr + i and the stride n, gp_corr_factors.hpp)
template <int MODE, class TERM, class DESC>
__global__ void __launch_bounds__(256) corr_batch_tiles_kernel(const DESC* __restrict__ descs, const CorrTile* __restrict__ tiles, const double* __restrict__ poses_lin,
                                                               const double* __restrict__ poses_eval, const int set, double* __restrict__ partials) {
  constexpr int NREG = MODE == MODE_LIN_GENERAL ? ACCG_SIZE : (MODE == MODE_ERR ? TERM::kErrRegs : 32);
  constexpr int STRIDE = MODE == MODE_LIN_GENERAL ? ACCG_STRIDE : ACC_STRIDE;
  const CorrTile t = tiles[blockIdx.x];
  // the two larger tables' entries are read in place (a private copy would go to scratch for the set-indexed corr[]); the LOAM table's 48 bytes are copied, as the
  // kernel they had to themselves copied them
  const std::conditional_t<TERM::kNeighbours == 1, const DESC&, const DESC> d = descs[t.factor];
  const TERM f = batch_term<TERM>(d);
  const Pose Tl = load_pose(poses_lin + 16 * (size_t)t.factor);
  const Pose Te = MODE == MODE_ERR ? load_pose(poses_eval + 16 * (size_t)t.factor) : Tl;
  double acc[NREG];
#pragma unroll
  for (int k = 0; k < NREG; k++) acc[k] = 0.0;
  const int* __restrict__ corr = d.corr[set];
  const int end = t.begin + t.count;
  for (int i = t.begin + threadIdx.x; i < end; i += 256) {
    const int c = corr[i];
    if (c < 0) continue;
    if constexpr (TERM::kNeighbours == 1)
      f.template accumulate<MODE>(i, (size_t)c, Tl, Te, acc);
    else  // (int[K][n], slot 0 the anchor)
      f.template accumulate<MODE>(i, corr + i, (size_t)d.n, Tl, Te, acc);
  }
  store_tile_sums_row<MODE>(acc, partials + (size_t)t.row * STRIDE);
}

// validate_correspondences over the LOAM tiles of a batch, into the set just searched; a tile of a member that did not enable it returns at once
__global__ void __launch_bounds__(256) loam_batch_validate_kernel(const LoamBatchDesc* __restrict__ descs, const CorrTile* __restrict__ tiles, const int set) {
  const CorrTile t = tiles[blockIdx.x];
  const LoamBatchDesc d = descs[t.factor];
  if (!d.validate) return;
  const int end = t.begin + t.count;
  for (int i = t.begin + threadIdx.x; i < end; i += 256) loam_validate_point(d.target_points, d.corr[set] + i, (size_t)d.n, d.k);
}

// part p takes the pose of its member
__global__ void corr_batch_part_poses_kernel(const int* __restrict__ part_member, int num_parts, const double* __restrict__ poses, double* __restrict__ part_poses) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 16 * num_parts) part_poses[i] = poses[16 * (size_t)part_member[i >> 4] + (i & 15)];
}

// member f's result = its part results added in part order (edge, then plane), `width` doubles each; one workgroup per member, completion word f behind it
__global__ void __launch_bounds__(128) corr_batch_combine_kernel(const int2* __restrict__ member_parts, const double* __restrict__ part_results, int width, double* __restrict__ out,
                                                                 const DoneFlags done) {
  const int2 m = member_parts[blockIdx.x];  // first part, number of parts (1 or 2)
  const int k = threadIdx.x;
  const bool mine = k < width;
  if (mine) {
    const double a = part_results[(size_t)m.x * width + k];
    out[(size_t)blockIdx.x * width + k] = m.y == 2 ? a + part_results[(size_t)(m.x + 1) * width + k] : a;
  }
  signal_done(done, blockIdx.x, mine);
}

}  // namespace gp

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------

struct gp_corr_batch {
  enum Kind { GICP = 0, ICP_POINT = 1, ICP_PLANE = 2, COLORED = 3, LOAM_EDGE = 4, LOAM_PLANE = 5, NUM_KINDS = 6 };  // the 1-NN kinds first: the order of the tile list
  static constexpr int kRecordDoubles = (int)(sizeof(gp_linearized6) / sizeof(double));
  hipStream_t stream = nullptr;
  int F = 0;                    // members = records
  int P = 0;                    // parts (>= F): what the tables below are indexed by
  bool combine = false;         // P > F: part poses in front of a pass, part results added behind it
  bool validate = false;        // a LOAM member enables the correspondence validation
  int num_tiles = 0;            // = rows of the partial sums
  long total_points = 0;
  int kind_begin[NUM_KINDS] = {0, 0, 0, 0, 0, 0}, kind_count[NUM_KINDS] = {0, 0, 0, 0, 0, 0};  // the tile list is ordered by kind: one tile launch per kind present
  int tiles_1nn = 0, tiles_knn = 0;                           // the tiles of the 1-NN kinds come first, those of the LOAM kinds behind them
  gp::DeviceArray d_search, d_descs, d_tiles, d_rows;         // search descriptors | CorrBatchDesc[P] | CorrTile[num_tiles] | FactorDesc[P] (tile_begin / tile_count: the finalize's)
  gp::DeviceArray d_loam_descs;                               // LoamBatchDesc[P] (the LOAM parts' entries)
  gp::DeviceArray d_colored_descs;                            // ColoredBatchDesc[P] (the colored GICP parts' entries)
  gp::DeviceArray d_part_member, d_member_parts;              // int[P] | int2[F]
  gp::DeviceArray d_part_poses[2], d_part_records, d_part_errors;  // combine: [P][16] lin | eval, gp_linearized6[P], double[P]
  gp::DeviceArray d_corr[2];                                  // int each: part p's correspondences (K rows of n) at its offset
  gp::DeviceArray d_partials_lin, d_partials_err;             // [num_tiles][ACCG_STRIDE] | [num_tiles][ACC_STRIDE]
  bool set_valid[2] = {false, false};
  // the synchronous host-pose forms and the LM graph's error evaluation: pose staging, results and completion words in host-mapped pinned memory
  gp::PinnedArray h_poses;
  gp::MappedResults res;  // F records (or errors) and F completion words
  gp::DeviceArray d_poses[2];

  long spin_us() const { return 200 + total_points / 500; }  // (the search is ~1 ns per point; the wait falls back to the stream behind it)

  // the tile launch of one kind, over that kind's stretch of the tile list (TERM: its per-point term, descs: the table the term is made from)
  template <int MODE, class TERM, class DESC>
  void launch_kind(Kind kind, const DESC* descs, const double* lin, const double* eval, int set, double* partials) {
    if (kind_count[kind] > 0)
      hipLaunchKernelGGL((gp::corr_batch_tiles_kernel<MODE, TERM, DESC>), dim3(kind_count[kind]), dim3(256), 0, stream, descs, d_tiles.as<gp::CorrTile>() + kind_begin[kind], lin, eval, set,
                         partials);
  }

  template <int MODE>
  int launch_tiles(const double* lin, const double* eval, int set, double* partials) {
    const gp::CorrBatchDesc* descs = d_descs.as<gp::CorrBatchDesc>();
    const gp::LoamBatchDesc* ldescs = d_loam_descs.as<gp::LoamBatchDesc>();
    launch_kind<MODE, gp::GicpTerm>(GICP, descs, lin, eval, set, partials);
    launch_kind<MODE, gp::IcpTerm<false>>(ICP_POINT, descs, lin, eval, set, partials);
    launch_kind<MODE, gp::IcpTerm<true>>(ICP_PLANE, descs, lin, eval, set, partials);
    launch_kind<MODE, gp::ColoredGicpTerm>(COLORED, d_colored_descs.as<gp::ColoredBatchDesc>(), lin, eval, set, partials);
    launch_kind<MODE, gp::LoamEdgeTerm>(LOAM_EDGE, ldescs, lin, eval, set, partials);
    launch_kind<MODE, gp::LoamPlaneTerm>(LOAM_PLANE, ldescs, lin, eval, set, partials);
    GP_HIP(hipGetLastError());
    return GP_OK;
  }

  // the members' poses [F][16] as the parts read them: the table itself when part p is member p, else gathered into d_part_poses[slot]
  int part_poses(const double* poses_dev, int slot, const double** out) {
    *out = poses_dev;
    if (!combine) return GP_OK;
    double* pp = d_part_poses[slot].as<double>();
    hipLaunchKernelGGL(gp::corr_batch_part_poses_kernel, dim3((16 * P + 255) / 256), dim3(256), 0, stream, d_part_member.as<int>(), P, poses_dev, pp);
    GP_HIP(hipGetLastError());
    *out = pp;
    return GP_OK;
  }

  int combine_parts(const double* part_results, int width, double* out, gp::DoneFlags done) {
    hipLaunchKernelGGL(gp::corr_batch_combine_kernel, dim3(F), dim3(128), 0, stream, d_member_parts.as<int2>(), part_results, width, out, done);
    GP_HIP(hipGetLastError());
    return GP_OK;
  }

  int issue_linearize(const double* poses_dev, bool rigid, int set, gp_linearized6* out, gp::DoneFlags done) {
    const double* pp = nullptr;
    GP_TRY(part_poses(poses_dev, 0, &pp));
    if (num_tiles > 0) {
      const gp::CorrTile* tiles = d_tiles.as<gp::CorrTile>();
      if (tiles_1nn > 0) GP_TRY(gp::launch_nearest_correspondences_batch(d_search.ptr, tiles, tiles_1nn, pp, set, stream));
      if (tiles_knn > 0) GP_TRY(gp::launch_nearest_k_correspondences_batch(d_search.ptr, tiles + tiles_1nn, tiles_knn, pp, set, stream));
      if (validate) {
        hipLaunchKernelGGL(gp::loam_batch_validate_kernel, dim3(tiles_knn), dim3(256), 0, stream, d_loam_descs.as<gp::LoamBatchDesc>(), tiles + tiles_1nn, set);
        GP_HIP(hipGetLastError());
      }
      if (rigid) GP_TRY(launch_tiles<gp::MODE_LIN>(pp, pp, set, d_partials_lin.as<double>()));
      else GP_TRY(launch_tiles<gp::MODE_LIN_GENERAL>(pp, pp, set, d_partials_lin.as<double>()));
    }
    set_valid[set] = true;
    if (!combine) return gp::launch_finalize_table(stream, d_rows.as<gp::FactorDesc>(), P, pp, d_partials_lin.as<double>(), out, !rigid, done);
    GP_TRY(gp::launch_finalize_table(stream, d_rows.as<gp::FactorDesc>(), P, pp, d_partials_lin.as<double>(), d_part_records.as<gp_linearized6>(), !rigid, {}));
    return combine_parts(d_part_records.as<double>(), kRecordDoubles, reinterpret_cast<double*>(out), done);
  }

  int issue_error(int set, const double* lin, const double* eval, double* out, gp::DoneFlags done) {
    const double *pl = nullptr, *pe = nullptr;
    GP_TRY(part_poses(lin, 0, &pl));
    GP_TRY(part_poses(eval, 1, &pe));
    if (num_tiles > 0) GP_TRY(launch_tiles<gp::MODE_ERR>(pl, pe, set, d_partials_err.as<double>()));
    if (!combine) return gp::launch_finalize_error_table(stream, d_rows.as<gp::FactorDesc>(), P, d_partials_err.as<double>(), out, done);
    GP_TRY(gp::launch_finalize_error_table(stream, d_rows.as<gp::FactorDesc>(), P, d_partials_err.as<double>(), d_part_errors.as<double>(), {}));
    return combine_parts(d_part_errors.as<double>(), 1, out, done);
  }

  // where the host-pose forms stage their poses and every synchronous form finds its results
  int alloc_staging() {
    const size_t pb = sizeof(double) * 16 * (size_t)F;
    for (int k = 0; k < 2; k++) GP_TRY(d_poses[k].alloc(pb));
    GP_TRY(h_poses.ensure(2 * pb));
    return res.ensure(sizeof(gp_linearized6) * (size_t)F, (size_t)F);
  }

  // host poses [F][16] -> d_poses[k] (through the pinned staging block; in stream order in front of the kernels that read them)
  int stage_poses(const double* poses_host, int k) {
    const size_t bytes = sizeof(double) * 16 * (size_t)F;
    char* h = static_cast<char*>(h_poses.ptr) + bytes * (size_t)k;
    memcpy(h, poses_host, bytes);
    GP_HIP(hipMemcpyAsync(d_poses[k].ptr, h, bytes, hipMemcpyHostToDevice, stream));
    return GP_OK;
  }
};

namespace gp {

int corr_batch_error_begin(gp_corr_batch* b, int set, const double* poses_lin_dev, const double* poses_eval_dev) {
  if (!b || !poses_lin_dev || !poses_eval_dev || (set != 0 && set != 1)) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch: error evaluation: null / set must be 0 or 1");
  if (!b->set_valid[set]) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch: error evaluation on a correspondence set that was never linearised");
  return b->issue_error(set, poses_lin_dev, poses_eval_dev, static_cast<double*>(b->res.out_dev), b->res.next());
}

int corr_batch_error_end(gp_corr_batch* b, double* out_host, long extra_spin_us) {
  GP_TRY(wait_done(b->res.words(), (size_t)b->F, b->res.seq, b->stream, b->spin_us() + extra_spin_us));
  memcpy(out_host, b->res.out.ptr, sizeof(double) * (size_t)b->F);
  return GP_OK;
}

}  // namespace gp

// The host tables of a batch under construction, in the stages gp_corr_batch_create_ex2 runs them: the parts list, the rows and the kind-ordered tile list, the
// per-part tables, the uploads.
struct BatchTables {
  // the parts in record order: a GICP / ICP / colored GICP member is one, a LOAM member its edge part and / or its plane part, in that order
  struct Part {
    const gp_corr_factor_core* core;
    int kind, member, k;
    const gp_loam_factor* loam;
  };
  std::vector<Part> parts;
  std::vector<int2> member_parts;  // [F] first part, number of parts
  // rows (= tiles) in part order, a part's rows contiguous; the tile LIST ordered by kind
  std::vector<gp::FactorDesc> rows;
  std::vector<long> corr_offset;
  std::vector<int> part_member;
  std::vector<gp::CorrTile> tiles;
  long total_corr = 0;
  std::vector<char> search;
  std::vector<gp::CorrBatchDesc> descs;
  std::vector<gp::LoamBatchDesc> ldescs;
  std::vector<gp::ColoredBatchDesc> cdescs;

  // the members of one kind, in record order behind those already there: push_parts(member, record index) appends the member's parts
  template <class F, class PUSH>
  int add_members(const F* const* members, int count, const char* what, const char* a_what, PUSH&& push_parts) {
    for (int i = 0; i < count; i++) {
      const F* f = members[i];
      if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, std::string("gp_corr_batch_create: null ") + what + " factor");
      // the keep-or-search decision of the update tolerances is host logic on a host pose: in a batch every linearise searches (the reference's default)
      if (f->upd.tol_rot != 0.0 || f->upd.tol_trans != 0.0)
        return gp::fail(GP_ERROR_INVALID_ARGUMENT, std::string("gp_corr_batch_create: ") + a_what + " factor with non-zero correspondence-update tolerances cannot join a batch");
      const int first = (int)parts.size();
      push_parts(f, (int)member_parts.size());
      member_parts.push_back(make_int2(first, (int)parts.size() - first));
    }
    return GP_OK;
  }

  int lay_out(gp_corr_batch* b) {
    const int P = (int)parts.size();
    b->F = (int)member_parts.size();
    b->P = P;
    b->combine = P != b->F;
    rows.assign((size_t)P, gp::FactorDesc{});
    corr_offset.resize((size_t)P);
    part_member.resize((size_t)P);
    std::vector<gp::CorrTile> by_kind[gp_corr_batch::NUM_KINDS];
    int row = 0;
    for (int p = 0; p < P; p++) {
      const Part& part = parts[(size_t)p];
      const int n = part.core->n;
      part_member[(size_t)p] = part.member;
      corr_offset[(size_t)p] = total_corr;
      total_corr += (long)part.k * n;
      b->total_points += n;
      b->validate = b->validate || (part.loam && part.loam->validation);
      rows[(size_t)p].n = n;
      rows[(size_t)p].tile_begin = row;
      for (int begin = 0; begin < n; begin += gp::kTilePoints) by_kind[part.kind].push_back(gp::CorrTile{p, begin, std::min(gp::kTilePoints, n - begin), row++});
      rows[(size_t)p].tile_count = row - rows[(size_t)p].tile_begin;
    }
    b->num_tiles = row;
    for (int k = 0; k < gp_corr_batch::NUM_KINDS; k++) {
      b->kind_begin[k] = (int)tiles.size();
      b->kind_count[k] = (int)by_kind[k].size();
      tiles.insert(tiles.end(), by_kind[k].begin(), by_kind[k].end());
    }
    b->tiles_1nn = b->kind_begin[gp_corr_batch::LOAM_EDGE];
    b->tiles_knn = (int)tiles.size() - b->tiles_1nn;
    if (b->tiles_knn == 0) b->validate = false;
    if (total_corr > 0x7fffffffl) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch_create: more than 2^31 - 1 correspondences in one batch");
    return GP_OK;
  }

  // the correspondence sets and the partial rows, then what the search and each kind's tile kernel read of part p (three tables [P] indexed by t.factor; a part
  // fills the entry of its own kind's table)
  int describe_parts(gp_corr_batch* b) {
    const int P = b->P;
    for (int k = 0; k < 2; k++) GP_TRY(b->d_corr[k].alloc(sizeof(int) * (size_t)std::max(total_corr, 1l)));
    GP_TRY(b->d_partials_lin.alloc(sizeof(double) * gp::ACCG_STRIDE * (size_t)std::max(b->num_tiles, 1)));
    GP_TRY(b->d_partials_err.alloc(sizeof(double) * gp::ACC_STRIDE * (size_t)std::max(b->num_tiles, 1)));
    search.resize(gp::corr_search_desc_bytes() * (size_t)P);
    descs.assign((size_t)P, gp::CorrBatchDesc{});
    ldescs.assign((size_t)P, gp::LoamBatchDesc{});
    cdescs.assign((size_t)P, gp::ColoredBatchDesc{});
    for (int p = 0; p < P; p++) {
      const Part& part = parts[(size_t)p];
      const gp_corr_factor_core* c = part.core;
      int* c0 = b->d_corr[0].as<int>() + corr_offset[(size_t)p];
      int* c1 = b->d_corr[1].as<int>() + corr_offset[(size_t)p];
      gp::fill_corr_search_desc(search.data(), p, c->grid, c->points, c->n, c->max_sq_dist, c0, c1, part.k);
      gp::CorrBatchDesc& d = descs[(size_t)p];
      if (part.kind == gp_corr_batch::COLORED) {
        cdescs[(size_t)p] = gp::ColoredBatchDesc{static_cast<const gp_colored_gicp_factor*>(c)->term, {c0, c1}};  // (the weight as it stands now; the cut-off went into the search table)
      } else if (part.kind == gp_corr_batch::GICP) {
        const gp::GicpTerm& t = static_cast<const gp_gicp_factor*>(c)->term;
        d.points = t.points, d.covs = t.covs, d.target_points = t.target_points, d.target_covs = t.target_covs;
      } else if (part.loam) {
        const gp::LoamDesc& t = static_cast<const gp_loam_part*>(c)->desc;
        ldescs[(size_t)p] = gp::LoamBatchDesc{t.points, t.target_points, {c0, c1}, c->n, part.k, part.loam->validation ? 1 : 0, 0};
      } else {
        const gp::IcpDesc& t = static_cast<const gp_icp_factor*>(c)->desc;
        d.points = t.points, d.target_points = t.target_points, d.target_normals = t.target_normals;
      }
      d.corr[0] = c0, d.corr[1] = c1;
    }
    return GP_OK;
  }

  int upload(gp_corr_batch* b) {
    GP_TRY(gp::upload(b->d_search, search));
    GP_TRY(gp::upload(b->d_descs, descs));
    GP_TRY(gp::upload(b->d_loam_descs, ldescs));
    GP_TRY(gp::upload(b->d_colored_descs, cdescs));
    GP_TRY(gp::upload(b->d_tiles, tiles));
    GP_TRY(gp::upload(b->d_rows, rows));
    GP_TRY(gp::upload(b->d_part_member, part_member));
    GP_TRY(gp::upload(b->d_member_parts, member_parts));
    if (b->combine) {
      for (int k = 0; k < 2; k++) GP_TRY(b->d_part_poses[k].alloc(sizeof(double) * 16 * (size_t)b->P));
      GP_TRY(b->d_part_records.alloc(sizeof(gp_linearized6) * (size_t)b->P));
      GP_TRY(b->d_part_errors.alloc(sizeof(double) * (size_t)b->P));
    }
    return GP_OK;
  }
};

extern "C" {

int gp_corr_batch_create(const gp_gicp_factor_t* const* gicp, int num_gicp, const gp_icp_factor_t* const* icp, int num_icp, gp_stream_t stream, gp_corr_batch_t** out) {
  return gp_corr_batch_create_ex2(gicp, num_gicp, icp, num_icp, nullptr, 0, nullptr, 0, stream, out);
}

int gp_corr_batch_create_ex(const gp_gicp_factor_t* const* gicp, int num_gicp, const gp_icp_factor_t* const* icp, int num_icp, const gp_loam_factor_t* const* loam, int num_loam,
                            gp_stream_t stream, gp_corr_batch_t** out) {
  return gp_corr_batch_create_ex2(gicp, num_gicp, icp, num_icp, loam, num_loam, nullptr, 0, stream, out);
}

int gp_corr_batch_create_ex2(const gp_gicp_factor_t* const* gicp, int num_gicp, const gp_icp_factor_t* const* icp, int num_icp, const gp_loam_factor_t* const* loam, int num_loam,
                             const gp_colored_gicp_factor_t* const* colored, int num_colored, gp_stream_t stream, gp_corr_batch_t** out) {
  if (!out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch_create: null out");
  *out = nullptr;
  if (num_gicp < 0 || num_icp < 0 || num_loam < 0 || num_colored < 0 || (num_gicp > 0 && !gicp) || (num_icp > 0 && !icp) || (num_loam > 0 && !loam) ||
      (num_colored > 0 && !colored))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch_create: bad arguments");
  if (num_gicp + num_icp + num_loam + num_colored == 0) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch_create: an empty batch");

  BatchTables t;
  using B = gp_corr_batch;
  GP_TRY(t.add_members(gicp, num_gicp, "GICP", "a GICP", [&](const gp_gicp_factor* f, int m) { t.parts.push_back({f, B::GICP, m, 1, nullptr}); }));
  GP_TRY(t.add_members(icp, num_icp, "ICP", "an ICP", [&](const gp_icp_factor* f, int m) { t.parts.push_back({f, f->plane ? B::ICP_PLANE : B::ICP_POINT, m, 1, nullptr}); }));
  GP_TRY(t.add_members(loam, num_loam, "LOAM", "a LOAM", [&](const gp_loam_factor* l, int m) {
    if (l->edge) t.parts.push_back({l->edge.get(), B::LOAM_EDGE, m, 2, l});
    if (l->plane) t.parts.push_back({l->plane.get(), B::LOAM_PLANE, m, 3, l});
  }));
  GP_TRY(t.add_members(colored, num_colored, "colored GICP", "a colored GICP", [&](const gp_colored_gicp_factor* f, int m) { t.parts.push_back({f, B::COLORED, m, 1, nullptr}); }));
  // the batch's one search launch is the 3-D one: a member that searches in XYZI (gp_colored_gicp_factor_set_intensity_grid) is refused, never searched in 3-D instead
  for (const BatchTables::Part& p : t.parts)
    if (p.core->xyzi)
      return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch_create: a colored GICP factor on an intensity grid (XYZI search) cannot join a batch yet: the batch searches in 3-D");
  for (const BatchTables::Part& p : t.parts)
    if (p.core->stream != (hipStream_t)stream) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch_create: every factor must have been created on the batch's stream");

  auto b = std::make_unique<gp_corr_batch>();
  b->stream = (hipStream_t)stream;
  GP_TRY(t.lay_out(b.get()));
  GP_TRY(t.describe_parts(b.get()));
  GP_TRY(t.upload(b.get()));
  GP_TRY(b->alloc_staging());
  *out = b.release();
  return GP_OK;
}

int gp_corr_batch_destroy(gp_corr_batch_t* b) { return gp_corr_destroy(b); }  // (the factors are the caller's)

int gp_corr_batch_size(const gp_corr_batch_t* b) { return b ? b->F : 0; }

int gp_corr_batch_stream(const gp_corr_batch_t* b, gp_stream_t* out) {
  if (!b || !out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch_stream: null");
  *out = (gp_stream_t)b->stream;
  return GP_OK;
}

int gp_corr_batch_sync(gp_corr_batch_t* b) {
  if (!b) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch_sync: null batch");
  GP_HIP(hipStreamSynchronize(b->stream));
  return GP_OK;
}

int gp_corr_batch_issue_linearize_dev(gp_corr_batch_t* b, const double* poses_dev, int rigid, int set, gp_linearized6* out_dev) {
  if (!b || !poses_dev || !out_dev || (set != 0 && set != 1)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch_issue_linearize_dev: null / set must be 0 or 1");
  return b->issue_linearize(poses_dev, rigid != 0, set, out_dev, {});
}

int gp_corr_batch_issue_compute_error_dev(gp_corr_batch_t* b, int set, const double* poses_lin_dev, const double* poses_eval_dev, double* out, unsigned long long* done_flags,
                                          unsigned long long done_seq) {
  if (!b || !poses_lin_dev || !poses_eval_dev || !out || (set != 0 && set != 1))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch_issue_compute_error_dev: null / set must be 0 or 1");
  if (!b->set_valid[set]) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch_issue_compute_error_dev: this correspondence set was never linearised");
  return b->issue_error(set, poses_lin_dev, poses_eval_dev, out, gp::DoneFlags{done_flags, done_seq});
}

// the synchronous host-pose forms (tests and callers outside the LM graph): set 0
int gp_corr_batch_linearize(gp_corr_batch_t* b, const double* poses_host, int rigid, gp_linearized6* out_host) {
  if (!b || !poses_host || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch_linearize: null");
  GP_TRY(b->stage_poses(poses_host, 0));
  const gp::DoneFlags done = b->res.next();
  GP_TRY(b->issue_linearize(b->d_poses[0].as<double>(), rigid != 0, 0, static_cast<gp_linearized6*>(b->res.out_dev), done));
  GP_TRY(gp::wait_done(b->res.words(), (size_t)b->F, done.seq, b->stream, b->spin_us()));
  memcpy(out_host, b->res.out.ptr, sizeof(gp_linearized6) * (size_t)b->F);
  return GP_OK;
}

int gp_corr_batch_compute_error(gp_corr_batch_t* b, const double* poses_lin_host, const double* poses_eval_host, double* out_host) {
  if (!b || !poses_lin_host || !poses_eval_host || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch_compute_error: null");
  if (!b->set_valid[0]) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_corr_batch_compute_error: correspondence set 0 was never linearised");
  GP_TRY(b->stage_poses(poses_lin_host, 0));
  GP_TRY(b->stage_poses(poses_eval_host, 1));
  GP_TRY(gp::corr_batch_error_begin(b, 0, b->d_poses[0].as<double>(), b->d_poses[1].as<double>()));
  return gp::corr_batch_error_end(b, out_host, 0);
}

}  // extern "C"
