/*
 * fmx.h — C-ABI of the MI355X-native scan-to-submap registration path for FORM.
 *
 * Drop-in boundary for form::Estimator's hot path (huangjuite/form).  Every entry
 * point names the reference interface it replaces (file:line under the reference's
 * form/ tree).  Plain pointers and sizes only; no exceptions cross this boundary;
 * errors are status codes + fmx_last_error().  One context = one HIP device + one
 * HIP stream; a context is NOT thread-safe (the reference's register_scan is also
 * driven from a single caller thread, bindings.cpp:147-179).
 *
 * Conventions
 *   - points: PointXYZf layout, 4 x float32 per point (x, y, z, pad), row-major
 *     organized R x C scan (form/utils.hpp:38-46; extraction.tpp:141-145).
 *   - poses: row-major 3x4 double [R | t] (gtsam::Pose3 = (R, t)).
 *   - planar features: 6 floats (x, y, z, nx, ny, nz); point features: 3 floats
 *     (form/feature/features.hpp:31-163 stores the same values as doubles).
 *   - Jacobian columns: GTSAM Pose3 tangent [w; v], right perturbation.
 *   - Augmented Hessian G: packed upper triangle, row-major, of [A b]^T [A b] with
 *     A, b whitened by 1/sigma (gtsam.hpp:67-86, 129-139).  Full mode: 13 x 13 ->
 *     91 doubles (A = [H_i H_j]); single-pose mode: 7 x 7 -> 28 doubles (A = H_j).
 */
#ifndef FMX_FMX_H_
#define FMX_FMX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMX_ABI_VERSION 1

typedef enum fmx_status {
  FMX_OK = 0,
  FMX_E_INVAL = 1, /* bad argument */
  FMX_E_SIZE = 2,  /* scan size != rows*cols (reference throws, extraction.tpp:141-145) */
  FMX_E_OOM = 3,   /* device allocation failed or a capacity was exceeded */
  FMX_E_HIP = 4,   /* HIP runtime error */
  FMX_E_STATE = 5, /* call out of order (e.g. match before map_build) */
  FMX_E_RANGE = 6, /* voxel coordinate outside the +-2^20 packed-key range */
  FMX_E_RCCL = 7   /* RCCL missing or a collective failed (multi-GPU only) */
} fmx_status;

/* form::FeatureExtractor::Params (form/feature/extraction.hpp:59-88). */
typedef struct fmx_extract_params {
  uint32_t neighbor_points;
  uint32_t num_sectors;
  double planar_threshold;
  uint32_t planar_feats_per_sector;
  uint32_t point_feats_per_sector;
  double radius;
  uint32_t min_points;
  double min_norm_squared;
  double max_norm_squared;
  int32_t num_columns;
  int32_t num_rows;
} fmx_extract_params;

/* form::Estimator::Params (form/form.hpp:42-56) flattened, plus device capacities. */
typedef struct fmx_params {
  fmx_extract_params extraction;
  double max_dist_matching;        /* MatcherParams, matcher.hpp:32-41 */
  double new_pose_threshold;
  uint32_t max_num_rematches;
  double planar_constraint_sigma;  /* ConstraintManager::Params, constraints.hpp:54-70 */
  int32_t disable_smoothing;       /* 0 (default): window smoothing; 1: single-pose ablation */
  int64_t max_num_keyscans;        /* KeyScanner::Params, keyscanner.hpp:55-64 */
  int64_t max_steps_unused_keyscan;
  uint32_t max_num_recent_scans;
  double keyscan_match_ratio;
  double min_dist_map;             /* KeypointMapParams, map.hpp:97-100 */
  /* device capacities (not in the reference: it allocates on demand) */
  uint64_t keypoint_pool_capacity; /* records per feature type kept in the window store */
  uint32_t max_pairs;              /* scans per submap (window size bound) */
  uint32_t voxel_subdivision;      /* device map cells = voxel width / this (1 or 2; 0 = 1):
                                      same matches; 2 tests fewer candidates per query but
                                      probes more cells (slower on C4/C5) */
} fmx_params;

typedef struct fmx_ctx fmx_ctx;

typedef struct fmx_feature_counts {
  uint32_t planar; /* planar features with a normal (extraction.tpp:99-118) */
  uint32_t point;  /* point features (extraction.tpp:120-129) */
  uint32_t planar_selected; /* planar indices before normal estimation */
} fmx_feature_counts;

int fmx_abi_version(void);
void fmx_default_params(fmx_params* p);

/* Estimator(const Params&) (form/form.hpp:74-76, form.cpp:31-38). */
fmx_status fmx_create(const fmx_params* p, int device, fmx_ctx** out);
void fmx_destroy(fmx_ctx* ctx);
const char* fmx_last_error(const fmx_ctx* ctx);

/* ---------------- stage 1: FeatureExtractor::extract ----------------------
 * Replaces FeatureExtractor::extract<PointXYZf> (extraction.hpp:99-101,
 * extraction.tpp:29-132).  xyzw: rows*cols float4; src_on_device != 0 means
 * xyzw is a device pointer on the context's device, else host memory.
 * The features stay device-resident as the context's current query set.
 * Host scans (here, in fmx_register_scan and fmx_next_scan): page-locked memory (from
 * fmx_scan_buffer, hipHostMalloc, hipHostRegister) is DMA'd directly; pageable memory
 * (the reference's std::vector<PointXYZf>, form.hpp:82-83) is first copied into the
 * context's pinned staging memory by a few helper threads and the caller, each part
 * DMA'd as soon as it is copied (FMX_STAGE_THREADS, default 3 helpers).  The pad
 * component must be 0, as every reference PointXYZf's is (utils.hpp:38-46). */
fmx_status fmx_extract(fmx_ctx* ctx, const float* xyzw, size_t n_points, uint64_t scan_idx,
                       int src_on_device, fmx_feature_counts* out);
/* A context-owned page-locked buffer of n_points float4 (PointXYZf layout) that a
 * caller assembling its scans (as FORM::add_lidar does, bindings.cpp:150-159) can fill
 * directly: passed as a host scan (src_on_device = 0) it is DMA'd with no staging copy.
 * Three buffers are handed out in turn: the one returned here is returned again by the
 * third next call, so a caller may fill scan k+1 while scan k registers.  Valid until
 * fmx_destroy, or until a later call asks for more points than that buffer holds: the
 * buffer is then reallocated (after draining every queued DMA from it), and an
 * announcement of a scan in the old buffer is withdrawn. */
fmx_status fmx_scan_buffer(fmx_ctx* ctx, size_t n_points, float** out);
/* Copy the last extraction to host (any pointer may be NULL):
 * planar[6*planar], planar_index[planar] (scan point index), point[3*point],
 * point_index[point], planar_mask[rows*cols] (compute_valid_points, 0/1). */
fmx_status fmx_extract_download(fmx_ctx* ctx, float* planar, uint32_t* planar_index,
                                float* point, uint32_t* point_index, uint8_t* planar_mask);

/* Replace the current query set (the scan being registered) with caller features. */
fmx_status fmx_set_queries(fmx_ctx* ctx, uint64_t scan_idx, const float* planar, uint32_t n_planar,
                           const float* point, uint32_t n_point);

/* Device-resident variants (no host round trip): float4 arrays (x, y, z, pad) that
 * already live on the context's device; normals likewise.  Same semantics as
 * fmx_set_queries / fmx_keypoints_add. */
fmx_status fmx_set_queries_device(fmx_ctx* ctx, uint64_t scan_idx, const float* planar_pos4,
                                  const float* planar_nrm4, uint32_t n_planar, const float* point_pos4,
                                  uint32_t n_point);

/* ---------------- stage 2: KeypointMap / VoxelMap / Matcher ---------------
 * Window keypoint store: KeypointMap::get(scan).push_back / insert_matches /
 * remove (map.tpp:95-126, 148-165).  Features are in the scan's local frame. */
fmx_status fmx_keypoints_add(fmx_ctx* ctx, uint64_t scan_idx, const float* planar,
                             uint32_t n_planar, const float* point, uint32_t n_point);
fmx_status fmx_keypoints_add_device(fmx_ctx* ctx, uint64_t scan_idx, const float* planar_pos4,
                                    const float* planar_nrm4, uint32_t n_planar, const float* point_pos4,
                                    uint32_t n_point);
fmx_status fmx_keypoints_remove(fmx_ctx* ctx, uint64_t scan_idx);
/* KeypointMap::to_voxel_map for both feature types (map.tpp:128-146, form.cpp:61-65):
 * builds the device voxel hash of every stored keypoint of scans[0..n) at the given
 * world poses.  Pair k of later calls refers to scans[k]. */
fmx_status fmx_map_build(fmx_ctx* ctx, const uint64_t* scans, const double* poses34,
                         uint32_t n_scans, double voxel_width);
/* Matcher<PlanarFeat>::match<0> + Matcher<PointFeat>::match<1> (matcher.hpp:67-112):
 * nearest map keypoint of every query at pose_j (VoxelMap::find_closest,
 * map.tpp:70-91), moved back to its scan's frame, accepted if d^2 < max_dist^2 and
 * bucketed per pair on the device.  counts_planar / counts_point (may be NULL):
 * K = n_scans accepted correspondences per pair.  With both NULL the call returns
 * without waiting for the device (once the map build's range check has been read);
 * the calls that read the results wait for them.
 * Deferred match: with both NULL on a large query set (>= 128k queries, windows of
 * <= 256 scans) the match is not launched yet.  Arguments are validated by this call
 * (FMX_E_INVAL / FMX_E_STATE are returned here, never by a later call).  If the next
 * consumer is fmx_linearize_matched at the same pose, match and linearization run as
 * ONE fused launch that writes no per-query results; its 7 x 7 sums are accumulated in
 * a different order than the two-step path (equal to 1e-10 relative, not bit for bit).
 * Any other reader (fmx_match_download, fmx_map_insert, fmx_linearize, ...) launches
 * the deferred match first, so its results are those of an immediate match.  Calls
 * that discard match results (fmx_set_queries*, fmx_extract, fmx_register_scan) drop
 * a deferred match without launching it. */
fmx_status fmx_match(fmx_ctx* ctx, const double pose_j34[12], double max_dist,
                     uint32_t* counts_planar, uint32_t* counts_point);
/* Per-query match results of the last fmx_match, planar queries then point
 * queries (any pointer may be NULL): pair[q] (-1 if not accepted), d2[q]
 * (DBL_MAX when no record lies within
 * max(max_dist, min_dist_map) of the query inside its 27 voxels; with both <= the
 * voxel width the search is bounded by them, otherwise it covers all 27 voxels, so a
 * finite d2 may exceed max_dist^2 — accept/insert decisions equal the reference's), pi[3q], ni[3q] (planar only). */
fmx_status fmx_match_download(fmx_ctx* ctx, int32_t* pair, double* d2, double* pi, double* ni);
/* KeypointMap::insert_matches (map.tpp:148-165): append every query of the last
 * match whose NN distance^2 > min_dist_map^2 to the store under the query scan. */
fmx_status fmx_map_insert(fmx_ctx* ctx, double min_dist_map, uint32_t* n_inserted);

/* ---------------- stage 3: FeatureFactor + DenseFactor::linearize ---------
 * Load correspondences directly (replacing the match output), pair-major:
 * plane rows p_i, n_i, p_j (3 doubles each) and point pairs p_i, p_j.
 * PlanePoint / PointPoint buffers, factor.hpp:43-130. */
fmx_status fmx_corr_set(fmx_ctx* ctx, uint32_t K, const uint32_t* n_plane,
                        const double* plane_pi, const double* plane_ni, const double* plane_pj,
                        const uint32_t* n_point, const double* point_pi, const double* point_pj);
/* The inverse of fmx_corr_set: the pair-major correspondences as the device holds them,
 * after a sorted fmx_match (a deferred match and a deferred row scatter are launched
 * first, as by every other reader) or after fmx_corr_set; FMX_E_STATE otherwise.  Nothing
 * is recomputed on the host.  sizes (may be NULL): K, the chunk count, the plane rows and
 * the point rows.  Every output pointer may be NULL and is then skipped with its
 * capacity; a call with only `sizes` asks for the capacities the next one needs.
 *   counts, pair_base  [2K]: per pair the plane rows then the point rows, and each
 *                      pair's first row per type; needs cap_pairs >= K
 *   chunk_range        [K + 1] (cap_pairs >= K): pair k owns chunks
 *                      [chunk_range[k], chunk_range[k + 1])
 *   chunks             [n_chunks][4] = type (0 plane, 1 point), pair, first row, end row:
 *                      per pair its plane chunks then its point chunks, 256 rows each;
 *                      needs cap_chunks >= n_chunks
 *   plane_* / point_*  the rows in device row order, 3 doubles per field and row as
 *                      fmx_corr_set takes them; cap_plane / cap_point in rows
 * A capacity that is too small: FMX_E_INVAL, and nothing is written. */
fmx_status fmx_corr_download(fmx_ctx* ctx, uint32_t sizes[4], uint32_t* counts, uint32_t* pair_base,
                             uint32_t* chunk_range, uint32_t cap_pairs, uint32_t* chunks, uint32_t cap_chunks,
                             double* plane_pi, double* plane_ni, double* plane_pj, uint32_t cap_plane,
                             double* point_pi, double* point_pj, uint32_t cap_point);
/* Host only (no context, no device): the form the pair sort of a match of n_planar +
 * n_point queries against K scans takes (form_amd/csrc/pair_sort_plan.hpp).
 * out = lanes per query (8 or 1), form (0 not sorted, 1 per-block histograms, 2 counts
 * scanned by the match's last block, 3 by the pair scatter), match blocks planar / point,
 * tiles planar / point, words scanned by the per-block form (else 0), scan launches
 * (0, 1 or 3).  FMX_E_INVAL: null out, or a scanned word count beyond 32 bits. */
fmx_status fmx_pair_sort_plan(uint32_t n_planar, uint32_t n_point, uint32_t K, int sorted, uint32_t out[8]);
/* A counter that changes whenever the context's correspondences may have been replaced
 * (fmx_match, fmx_corr_set, fmx_register_scan): a caller caching fmx_linearize results per
 * set of poses (fmx_seam.hpp's FmxBatch) keys its cache on it as well. */
fmx_status fmx_corr_generation(fmx_ctx* ctx, uint64_t* gen);
/* DenseFactor::linearize of every pair's FeatureFactor (gtsam.hpp:67-86,
 * factor.cpp:142-186): poses_i / poses_j are K x 12.  G: K x 91 (single_pose=0)
 * or K x 28 (single_pose=1); err: K x 1 = 0.5*||r/sigma||^2 (may be NULL). */
fmx_status fmx_linearize(fmx_ctx* ctx, const double* poses_i34, const double* poses_j34,
                         double sigma, int single_pose, double* G, double* err);
/* Pair moments: DenseFactor::linearize "once, evaluated anywhere".  Every row's whitened
 * [H_i H_j -r] is linear in 16 per-row features taken at reference poses (plane rows:
 * r0 = n.(q0 - p_i), n x q0, n, n (x) p_j with q0 = p_j in frame i; point rows: the world
 * residual e0, p_i, p_j, 1), so a pair's 13 x 13 information at ANY poses is C Phi C^T
 * with Phi = sum over its rows of phi phi^T.  fmx_moments: Phi of every pair of the
 * context's correspondences (fmx_match / fmx_corr_set) at reference poses
 * poses_i[k], poses_j[k] (K x 12 each), on the device (one launch).  mom: K x 272 =
 * per pair the packed upper 16 x 16 of the plane rows, then of the point rows. */
fmx_status fmx_moments(fmx_ctx* ctx, const double* ref_i34, const double* ref_j34, double* mom);
/* Host only (no context, no device): the packed 13 x 13 G (K x 91, may be NULL) and
 * errors 0.5 ||r/sigma||^2 (K, may be NULL) of K pairs at poses (poses_i[k],
 * poses_j[k]) from their moments mom (K x 272) taken at (ref_i[k], ref_j[k]) — equal to
 * fmx_linearize at the same poses up to rounding (gtsam.hpp:67-86, factor.cpp:30-128). */
fmx_status fmx_moments_contract(uint32_t K, const double* mom, const double* ref_i34, const double* ref_j34,
                                const double* poses_i34, const double* poses_j34, double sigma, double* G,
                                double* err);
/* NoiseModelFactor::error of every pair (FeatureFactor::evaluateError without
 * Jacobians), err: K x 1. */
fmx_status fmx_error(fmx_ctx* ctx, const double* poses_i34, const double* poses_j34,
                     double sigma, double* err);
/* The single-pose ablation's whole linear system at X(j) = pose_j34 (X(i) fixed at
 * the built map's poses; fused with a deferred fmx_match at the same pose, see
 * fmx_match): sum over every accepted match of the last fmx_match of the
 * 7 x 7 [H_j b]^T [H_j b] — what GTSAM's LM eliminates from get_single_graph's
 * BinaryFactorWrapper<FeatureFactor>s (constraints.cpp:235-250, gtsam.hpp:40-54,
 * 144-170) — in one launch over the match outputs in query order.  out[0..27]: the
 * packed upper 7 x 7, out[28]: the error 0.5 ||r/sigma||^2. */
fmx_status fmx_linearize_matched(fmx_ctx* ctx, const double pose_j34[12], double sigma, double out[29]);

/* Point-set registration against the built map in the single-pose formulation (the
 * 2M-point C5 configuration): from pose_init, iterate
 *   Matcher::match at X (matcher.hpp:67-112) -> the summed 7 x 7 [H_j b]^T [H_j b]
 *   (gtsam.hpp:67-86, 144-170; all-reduced over the communicator's ranks, below) ->
 *   Gauss-Newton step H dx = g -> X <- X Exp(dx)
 * until ||dx|| < threshold (form.cpp:83-88's break) or max_iters iterations.  The whole
 * loop runs in libfmx (on large query sets each iteration is one fused launch); every
 * rank of a communicator computes the identical iterate.  pose_out: the result, *iters
 * (may be NULL): the iterations run.  FMX_E_STATE if a system is singular. */
fmx_status fmx_register_points(fmx_ctx* ctx, const double pose_init34[12], double max_dist, double sigma,
                               uint32_t max_iters, double threshold, double pose_out34[12], uint32_t* iters);

/* ---------------- multi-GPU: the sharded C5 path -----------
 * One rank per GPU, each with the same voxel map and a contiguous shard of the
 * queries.  fmx_comm_unique_id on one rank; the caller shares the 128 bytes (e.g. a
 * torch.distributed broadcast); fmx_comm_init on every rank (collective).  From then
 * on the context's linearization sums — fmx_linearize_matched's 7 x 7 system and
 * fmx_linearize / fmx_error's per-pair G — are all-reduced (fp64 sum) over the ranks
 * with RCCL on the context's HIP stream, device buffer to device buffer, before they
 * reach the host, so every rank returns the identical global system.  The reference
 * has no multi-device path; this is the north star's "RCCL all-reduce of the normal
 * equations over xGMI".  RCCL is loaded on first use (FMX_E_RCCL if absent).  A wait for
 * an all-reduce is bounded: it polls the stream and ncclCommGetAsyncError and, after
 * FMX_COMM_TIMEOUT_S seconds (environment, default 60), aborts the communicator and
 * returns FMX_E_RCCL.  The communicator is gone then, and every later sharded call
 * (fmx_linearize_matched, fmx_linearize / fmx_error, fmx_register_points) also returns
 * FMX_E_RCCL until fmx_comm_init attaches a new one: this rank holds only a shard of the
 * queries, so a rank-local system must never stand in for the global one. */
fmx_status fmx_comm_unique_id(uint8_t id[128]);
fmx_status fmx_comm_init(fmx_ctx* ctx, const uint8_t id[128], int nranks, int rank);

/* ---------------- host adapter: Estimator::register_scan -------------------
 * form::Estimator::register_scan (form/form.hpp:82-83, form.cpp:40-114): predict,
 * extract, map build, ICP loop (match + LM), final LM, insert_matches, keyscan
 * selection, marginalization.  The smoother runs in ConstraintManager's default
 * smoothing mode (LM over every window pose, constraints.cpp:103-118, 252-308,
 * marginal LinearContainerFactors, constraints.cpp:120-203) or, with
 * params.disable_smoothing, in the single-pose ablation (constraints.cpp:103-111,
 * 235-250).  Every FeatureFactor linearization runs on the device. */
fmx_status fmx_register_scan(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                             fmx_feature_counts* out);
/* Pipelined extraction (no reference counterpart; an fmx throughput option).
 * Announces the scan that will FOLLOW the one passed to the next fmx_register_scan:
 * that call extracts it (FeatureExtractor::extract, extraction.tpp:29-132) on a side
 * stream while it registers its own scan, and the register_scan of this scan then
 * skips its extraction.  Results are identical either way: extraction depends only on
 * the scan.  The scan may be device-resident (src_on_device = 1) or host memory (0: a
 * pageable scan's staging copy starts at once on the helper threads, and the scan is
 * DMA'd and extracted on the side stream as soon as that copy has finished); it must
 * stay unchanged until its own fmx_register_scan returns.  That call must pass the
 * same pointer with the same src_on_device, else the queued extraction is discarded
 * and the scan extracted in the call.  xyzw = NULL withdraws the announcement.  A
 * withdrawing or replacing call returns only once the staging copy of a withdrawn or
 * replaced pageable scan has finished: from then on its memory is no longer read. */
fmx_status fmx_next_scan(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device);
/* ---------------- scan deskewing (no reference counterpart) ------------------
 * The reference computes the sweep's start and end stamps and never uses them
 * (python/bindings.cpp:151-152).  Opt-in constant-velocity motion compensation of the
 * sweep ahead of feature extraction: column c of the organized scan, sampled at sweep
 * fraction s_c (default c / cols), is moved to the sensor frame at MID-sweep,
 *   p' = Exp((s_c - 0.5) xi) p,   xi = [w; v] the body-frame twist per scan period
 * (GTSAM Pose3 tangent order), in fp64, rounded once to fp32; a dropout (x = y = z = 0)
 * stays 0 and the caller's scan is never written.  The reference fraction 0.5 is fixed:
 * referred to the sweep start the estimator's own twist feeds back with gain 1.5 and
 * diverges (DESIGN.md §Scan deskewing).  With deskewing on, fmx_register_scan of scan j uses
 *   1. the one-shot twist of fmx_deskew_set_twist (IMU / wheel odometry), if one was
 *      given since the previous registration; else
 *   2. Log(T_{j-2}^-1 T_{j-1}) of the window's current estimates, if it holds both
 *      (the two poses predict_next reads, constraints.cpp:71-101); else
 *   3. initial_twist (scans 0 and 1: a platform that starts at rest passes 0).
 * The pose estimated for the scan (fmx_current_pose) is then the sensor pose at
 * mid-sweep, and the features of fmx_extract_download are in that frame.  Never
 * configured, or enable = 0: every entry point behaves exactly as without this block. */
typedef struct fmx_deskew_params {
  int32_t enable;               /* 0 = off */
  double initial_twist[6];      /* [w; v] per scan period; default 0 */
  const float* column_fraction; /* cols floats in [0,1], copied; NULL = c/cols */
} fmx_deskew_params;
/* Before the first fmx_register_scan of the context (FMX_E_STATE afterwards); a fraction
 * outside [0,1] or non-finite: FMX_E_INVAL.  Allocates every buffer deskewing needs. */
fmx_status fmx_deskew_configure(fmx_ctx* ctx, const fmx_deskew_params* p);
/* One-shot twist for the next fmx_register_scan (overrides the constant-velocity one).
 * If that scan was announced (fmx_next_scan) and already extracted, the extraction is
 * dropped and redone in its own fmx_register_scan.  FMX_E_STATE unless deskewing is on. */
fmx_status fmx_deskew_set_twist(fmx_ctx* ctx, const double twist[6]);
/* Twist the last fmx_register_scan used; *source = 0 none/off, 1 initial, 2 constant
 * velocity, 3 caller.  Either pointer may be NULL. */
fmx_status fmx_deskew_last(fmx_ctx* ctx, double twist[6], int* source);
/* Stand-alone: deskew one rows*cols scan with a given twist (the same kernel, the
 * configured column fractions if any); in / out are host or device memory, out must not
 * alias in (FMX_E_INVAL).  Returns once out is written. */
fmx_status fmx_deskew(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                      const double twist[6], float* out_xyzw, int dst_on_device);

/* ---------------- unorganized clouds (no reference counterpart) --------------
 * The reference copies the measurement's points in order and hands them to the estimator
 * as the organized scan (python/bindings.cpp:150-156): evalio delivers rows*cols points,
 * row-major, with zeros for missing returns.  A sensor driver (Velodyne, Hesai, a ROS
 * PointCloud2) delivers an unordered list of returns instead, each with a ring index and
 * a time.  Opt-in stage "cloud in, organized device scan out", ahead of the unchanged
 * pipeline (DESIGN.md §Unorganized clouds).  For each point, all in fp64 on the fp32
 * coordinates:
 *   skipped (counted invalid) when x, y or z is not finite or x = y = z = 0;
 *   u = (atan2(y, x) - azimuth_offset) * cols / 2pi, negated when clockwise;
 *   col = floor(u + 0.5) mod cols (column c is centred on azimuth c * 2pi / cols);
 *   row = ring_to_row[ring] (identity without a table; a ring at or past the table, or
 *         mapped to -1: off-grid), or, in elevation mode, the table entry nearest to
 *         atan2(z, sqrt(x*x + y*y)), a tie to the lower row, off-grid when beyond an
 *         outermost entry by more than half the spacing to that entry's neighbour.
 * Of the points of one cell the one with the smallest r2 = (x*x + y*y) + z*z (fp32, that
 * order, no contraction) stays, the lowest input index among equal r2; the others count
 * as displaced.  The result does not depend on the order the device's threads run in.
 * Never configured, or enable = 0: every other entry point behaves exactly as without
 * this block. */
typedef enum fmx_row_source { FMX_ROW_RING = 0, FMX_ROW_ELEVATION = 1 } fmx_row_source;
typedef struct fmx_organize_params {
  int32_t enable;             /* 0 = off */
  int32_t row_source;         /* fmx_row_source */
  const double* elevation;    /* elevation mode: rows angles in radians, strictly monotonic, copied */
  const int32_t* ring_to_row; /* ring mode: n_rings rows (-1 = off-grid), copied; NULL = identity */
  uint32_t n_rings;
  double azimuth_offset;      /* azimuth of the centre of column 0, radians */
  int32_t clockwise;          /* 1: columns count clockwise (seen from above) */
} fmx_organize_params;
/* rows and cols are the context's extraction parameters.  Before the first registration of
 * the context (FMX_E_STATE afterwards).  FMX_E_INVAL: an elevation table that is not
 * strictly monotonic or holds a non-finite value, elevation mode without a table, a
 * ring_to_row entry >= rows (or < -1), a non-finite offset.  Allocates every buffer the
 * stage needs, sized for clouds of up to 2 * rows * cols points (a larger cloud grows the
 * device copies of a host cloud once). */
fmx_status fmx_organize_configure(fmx_ctx* ctx, const fmx_organize_params* p);
typedef struct fmx_cloud {
  const float* xyzw;           /* n * (x, y, z, pad) */
  size_t n;
  const uint16_t* ring;        /* n ring indices; required in ring mode, else may be NULL */
  const float* sweep_fraction; /* n sweep fractions in [0,1] (clamped), or NULL */
  int32_t on_device;           /* all three arrays in device (1) or host (0) memory */
} fmx_cloud;
typedef struct fmx_organize_counts {
  uint32_t placed;    /* cells filled */
  uint32_t displaced; /* lost their cell to a nearer (or equal and earlier) point */
  uint32_t off_grid;
  uint32_t invalid;   /* the four sum to n */
} fmx_organize_counts;
/* Stand-alone: organize one cloud.  out_xyzw: rows*cols points, winners copied bit for bit
 * with pad 0, empty cells all 0; out_index: per cell the winner's input index, 0xFFFFFFFF
 * for an empty cell; out_fraction: per cell the winner's sweep fraction, 0 for an empty
 * cell (left unwritten when the cloud has none).  The three outputs are device memory when
 * dst_on_device, else host memory; any of them and counts may be NULL.  Returns once they
 * are written.  FMX_E_STATE unless the stage is configured and enabled; FMX_E_INVAL for a
 * NULL cloud, ring = NULL in ring mode, n >= 2^32, n = 0 with a non-NULL array, n > 0
 * with xyzw = NULL. */
fmx_status fmx_organize(fmx_ctx* ctx, const fmx_cloud* cloud, float* out_xyzw, int dst_on_device,
                        uint32_t* out_index, float* out_fraction, fmx_organize_counts* counts);
/* Organize the cloud into the context's next device buffer (two in rotation), then exactly
 * fmx_register_scan of that buffer with src_on_device = 1.  With deskewing on and
 * sweep_fraction given, every point is deskewed with its own fraction (the per-cell plane);
 * without fractions, with the configured column table or c / cols.  Twist selection,
 * fmx_deskew_last, fmx_current_pose and fmx_last_stats as for fmx_register_scan.  A scan
 * announced with fmx_next_scan is the documented pointer mismatch: its queued extraction
 * is discarded.  Clouds cannot be announced ahead of time (the organizer is not
 * pipelined).  Either counts pointer may be NULL. */
fmx_status fmx_register_cloud(fmx_ctx* ctx, const fmx_cloud* cloud, fmx_feature_counts* feature_counts,
                              fmx_organize_counts* organize_counts);
/* Stand-alone: fmx_deskew with one sweep fraction per point of the rows*cols scan
 * (fraction: n_points floats in [0,1], in the memory kind of xyzw) instead of one
 * per column; equal fractions give fmx_deskew's bits.  Needs no configuration. */
fmx_status fmx_deskew_cells(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                            const float* fraction, const double twist[6], float* out_xyzw, int dst_on_device);

/* ---------------- dense voxel map (no reference counterpart) -------------------
 * The reference's users get a map of the registered points from scripts/rerun_map.py:
 * every n-th scan of the trajectory, range-gated (dist2 > min2 and dist2 < max2), rotated
 * into the world and concatenated on the host.  Opt-in, on the device: a fixed-capacity
 * hash of world voxels that the registered scans are integrated into (DESIGN.md §Dense
 * map).  Integrating n points p_i at pose T = [R | t] does, for each point:
 *   invalid       x, y or z not finite, or x = y = z = 0;
 *   gated         r2 = (x*x + y*y) + z*z (fp32, that order, no contraction), widened to
 *                 double, unless r2 > min_norm_squared && r2 < max_norm_squared (both strict);
 *   world point   w_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k in fp64;
 *   voxel         c_k = floor(w_k / voxel_width) in fp64; out_of_range unless every
 *                 |c_k| < 2^20 - 1.
 * A voxel keeps `hits`, the number of valid in-range points that ever fell into it, and
 * one representative: the point with the smallest (integration number, input index), its
 * fp64 world point stored once and never changed.  The first integration to see a voxel
 * owns it, within it the lowest index; later ones only add to hits.  The map's content
 * does not depend on the order the device's threads run in.  The table has the smallest
 * power of two >= 2 * max_voxels slots; an integration is refused (FMX_E_OOM, nothing
 * launched, nothing changed) unless voxels + n <= max_voxels, so no point is ever dropped
 * for lack of room.  The table never grows; the map is pruned only by the rolling block
 * below, and only for a caller who asks for it.  Never configured, or
 * enable = 0: every other entry point behaves exactly as without this block. */
typedef struct fmx_dense_params {
  int32_t enable;            /* 0 = off */
  double voxel_width;        /* > 0, finite */
  uint64_t max_voxels;       /* > 0; FMX_E_INVAL past 2^29 */
  double min_norm_squared;   /* both 0: the context's extraction values */
  double max_norm_squared;
  uint32_t every;            /* register path: integrate every n-th registered scan; 0 = 1 */
} fmx_dense_params;
typedef struct fmx_dense_counts {
  uint32_t added;        /* new voxels */
  uint32_t merged;       /* valid points that did not become a representative */
  uint32_t gated;
  uint32_t out_of_range;
  uint32_t invalid;      /* the five sum to n */
} fmx_dense_counts;
/* Before the first registration and the first integration of the context (FMX_E_STATE
 * afterwards).  Allocates the table (44 B per slot; 52 B once carving is enabled, further
 * down) and every per-scan buffer: FMX_E_OOM
 * when that fails.  FMX_E_INVAL: a voxel width that is not finite and positive, max_voxels
 * 0 or past 2^29, a gate that is NaN, negative or empty (min >= max). */
fmx_status fmx_dense_configure(fmx_ctx* ctx, const fmx_dense_params* p);
/* Stand-alone: integrate n_points < 2^32 points (host or device memory) at pose34 under the
 * caller's scan_idx.  Returns once the counts are in (counts may be NULL).  FMX_E_STATE
 * unless the map is configured and enabled; FMX_E_INVAL for a non-finite pose or NULL points
 * with n_points > 0; FMX_E_OOM by the capacity rule above. */
fmx_status fmx_dense_integrate(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                               const double pose34[12], uint64_t scan_idx, fmx_dense_counts* counts);
/* Register path: with the map on, a successful fmx_register_scan or fmx_register_cloud of
 * every `every`-th scan (scans 0, every, 2 every, ...) integrates the scan the extractor saw
 * (the deskewed scan with deskewing on, the organized scan of a cloud: index is then the
 * cell) at the pose fmx_current_pose returns after that call, under the scan's own index.
 * The integration has read the scan when the registration returns.  A capacity refusal
 * never fails the registration.  What the last registration did: its counts and
 * *integrated = 1 integrated, 0 skipped by `every` (or the map is off), -1 refused for
 * capacity.  Either pointer may be NULL. */
fmx_status fmx_dense_last(fmx_ctx* ctx, fmx_dense_counts* counts, int* integrated);
/* out = {voxels, max_voxels, integrations, slots}; all 0 when never configured. */
fmx_status fmx_dense_stats(fmx_ctx* ctx, uint64_t out[4]);
/* The voxels with hits >= min_hits (0 is taken as 1), in no particular order: xyz[3n] the
 * representative's world point, scan[n] the scan_idx of the integration that owns the voxel,
 * index[n] the representative's input index, hits[n].  Two calls, as for the keypoint map's
 * download: with all four buffers NULL *n receives the count; with buffers (any may be
 * NULL and is then skipped) *n is the capacity on entry (FMX_E_SIZE if too small, nothing
 * written) and the count on return. */
fmx_status fmx_dense_download(fmx_ctx* ctx, uint32_t min_hits, double* xyz, uint64_t* scan, uint32_t* index,
                              uint32_t* hits, uint32_t* n);
/* Empty the map; the integration counter restarts at 0.  Forgets the rolling centre and
 * leaves the spill alone (below). */
fmx_status fmx_dense_clear(fmx_ctx* ctx);

/* ---------------- rolling the dense voxel map ----------------------------------
 * Bounded memory for an unbounded stream: the map keeps what lies in a box around a centre,
 * everything else leaves the device and goes to the caller (DESIGN.md §Dense map, Rolling).
 * A roll takes a centre c (three finite doubles) and half-extents half (three uint32, in
 * voxels, each <= 2^21).  The centre voxel is cc_k = floor(c_k / voxel_width) in fp64, the
 * integration's own expression; FMX_E_INVAL unless every |cc_k| < 2^20 - 1.  A stored
 * voxel's coordinates v_k are decoded from its key; it is inside iff |v_k - cc_k| <= half_k
 * on all three axes, in 64-bit integers.  Every voxel outside is evicted: its (xyz, scan_idx,
 * index, hits), the fields fmx_dense_download returns, go to the caller in no particular
 * order and the voxel leaves the table.  Every voxel inside stays, bit for bit.  Afterwards
 * `voxels` is the number kept and the capacity rule uses it; the integration counter is
 * unchanged; a later integration that sees an evicted voxel again opens it as a new voxel
 * (fmx_upload_voxels, below, puts evicted voxels back first and so avoids that).
 * The content after a roll does not depend on the order the device's threads run in.
 * All of these: FMX_E_STATE unless the dense map is configured and enabled (fmx_roll_stats
 * excepted); FMX_E_INVAL for a null centre, a non-finite centre, a centre voxel out of
 * range or half_k > 2^21.  A context that calls none of them allocates and launches nothing
 * for them. */
typedef struct fmx_roll_params {
  int32_t enable;     /* 0: the register path never rolls */
  uint32_t half[3];   /* box half-extents in voxels */
  double step;        /* metres, finite, >= 0 */
  int32_t spill;      /* 1: keep evicted voxels for fmx_roll_drain; 0: discard them */
} fmx_roll_params;
/* Register path, opt-in (enable = 1): at the start of the registration of scan j >= 1, before
 * it is decided whether scan j is integrated, let p be the translation of the pose
 * fmx_current_pose returns at that moment (scan j - 1's final pose).  With no centre recorded,
 * p is recorded and nothing rolls.  Otherwise the map rolls about p, and p is recorded, iff
 * max_k |p_k - centre_k| >= step (fp64), or scan j is due by `every` and voxels + n >
 * max_voxels.  A p whose centre voxel is out of range, or a failed allocation, skips the roll;
 * neither fails the registration.  Evicted voxels go to the context's host spill, or nowhere
 * when spill = 0.  Estimation is untouched.  May be called at any time once the map is on;
 * forgets the recorded centre.  FMX_E_INVAL for a negative or non-finite step. */
fmx_status fmx_roll_configure(fmx_ctx* ctx, const fmx_roll_params* p);
/* out = {inside, outside} of the box; changes nothing. */
fmx_status fmx_roll_count(fmx_ctx* ctx, const double centre[3], const uint32_t half[3], uint64_t out[2]);
/* Stand-alone roll.  With any buffer non-NULL *n is the capacity on entry (FMX_E_SIZE if too
 * small: the map and the buffers stay untouched) and the evicted count on return; buffers
 * left NULL are skipped.  With all four NULL the evicted voxels are discarded; n may then be
 * NULL, or receives the count.  FMX_E_OOM, nothing changed, when a device allocation fails. */
fmx_status fmx_roll_evict(fmx_ctx* ctx, const double centre[3], const uint32_t half[3], double* xyz, uint64_t* scan,
                          uint32_t* index, uint32_t* hits, uint32_t* n);
/* The host spill of the register path's rolls, by fmx_dense_download's two-call protocol; a
 * successful filling call empties it.  It holds scan_idx values: fmx_dense_clear does not
 * invalidate it. */
fmx_status fmx_roll_drain(fmx_ctx* ctx, double* xyz, uint64_t* scan, uint32_t* index, uint32_t* hits, uint32_t* n);
/* out = {rolls, voxels evicted in total, voxels now in the spill, kept by the last roll,
 * evicted by the last roll, index of the scan whose registration ran the last roll}: the
 * register path's rolls only; all 0 when never used. */
fmx_status fmx_roll_stats(fmx_ctx* ctx, uint64_t out[6]);

/* ---------------- carving the dense voxel map: per-voxel ray miss counts ---------
 * A voxel of the dense map is never contradicted once it exists, so whatever moved while the
 * map was built stays in it.  Opt-in: every integrated point also casts a ray from the sensor
 * to itself, and a stored voxel keeps `misses`, the number of rays that passed through it
 * (DESIGN.md §Dense map, Carving).  Nothing is ever removed from the table: a download
 * filters by misses against hits on the way out.  All of it is exact, fp64 without
 * contraction, one rounding per written operation (tests/carve_ref.py restates it):
 *   ray      a point i of an integration that is valid, inside the dense gate and in range
 *            (it counts as added or merged), with r2 < max_norm_squared (the same fp32 r2,
 *            widened) and i % ray_stride == 0 on the input index;
 *   ends     e = the point's world point (the integration's expression), o = the pose's
 *            translation; w the voxel width; a_k = floor(o_k / w), b_k = floor(e_k / w), so b
 *            is the point's own voxel.  Unless every |a_k| < 2^20 - 1 the call casts no ray;
 *   walk     cur = a, then exactly S = sum_k |b_k - a_k| steps: v_0 = a ... v_S = b.  With
 *            d_k = e_k - o_k and s_k = +1 if b_k > a_k else -1: an axis with cur_k != b_k has
 *            tau_k = ((double)(cur_k + (s_k > 0 ? 1 : 0)) * w - o_k) / d_k, an axis with
 *            cur_k == b_k has tau_k = +inf; the walk steps cur_k += s_k on the axis with the
 *            smallest tau_k, the lowest k among equal ones;
 *   examined the voxels v_s with 0 <= s <= S - 1 - margin.  Each is looked up in the table
 *            (find only: home slot mix64 of the key & (slots - 1), linear probing up to the key
 *            or an empty slot).  Absent: nothing.  Present, and a point of this same
 *            integration fell into it (any valid in-range point, cast or not): exempt, nothing
 *            (a surface seen at a grazing angle does not carve itself).  Otherwise its misses
 *            grow by one.
 * The result is a sum over a set of (ray, voxel) pairs that the definition fixes: it does
 * not depend on the order the device's threads run in.  A roll keeps a kept voxel's misses
 * and hands an evicted voxel's over; fmx_dense_clear zeroes them.  Never configured: every
 * other entry point behaves, allocates and launches exactly as without this block, and
 * misses reads 0 wherever it is returned. */
typedef struct fmx_carve_params {
  int32_t enable;            /* 0: integrations stop carving (the counts so far stay) */
  double max_norm_squared;   /* the carve gate; 0: the dense gate's max_norm_squared */
  uint32_t margin;           /* voxels in front of the return that are left alone */
  uint32_t ray_stride;       /* 0 = 1 */
  uint32_t every;            /* carve the integrations whose number is a multiple of this; 0 = 1 */
} fmx_carve_params;
typedef struct fmx_carve_counts {
  uint32_t rays;
  uint64_t steps;            /* voxels examined */
  uint64_t misses;           /* ... present and not exempt */
  uint64_t exempt;           /* ... present and exempt */
} fmx_carve_counts;
/* At any time once the dense map is on (FMX_E_STATE otherwise); replaces the earlier
 * parameters.  The first enabling call on a map allocates and zeroes the two arrays (8 B per
 * slot on top of the table's 44): FMX_E_OOM, the map and the earlier parameters as they were,
 * when that fails.  FMX_E_INVAL: p NULL, a NaN or negative gate.  Reconfiguring the dense map
 * drops the arrays and turns carving off. */
fmx_status fmx_carve_configure(fmx_ctx* ctx, const fmx_carve_params* p);
/* Stand-alone: the rays of n_points < 2^32 points (host or device memory) at pose34 against
 * the map as it stands, by the configured gate, margin and stride (`enable` and `every` play
 * no part).  Integrates nothing, and nothing is exempt.  Returns once the counts are in
 * (counts may be NULL).  FMX_E_STATE unless carving has been enabled on this map; FMX_E_INVAL
 * for a non-finite pose or NULL points with n_points > 0. */
fmx_status fmx_carve_rays(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                          const double pose34[12], fmx_carve_counts* counts);
/* With carving enabled, fmx_dense_integrate and the register path's integrations whose
 * integration number (0, 1, 2, ... since the last clear) is a multiple of `every` carve after
 * integrating: the scan the integration saw, at the same pose.  The call returns once the
 * rays have read the scan.  A registration never fails because of carving.  What the last
 * such call (integrate, register_scan, register_cloud) did: its counts and *carved = 1 if it
 * carved, else 0 with counts all 0.  Either pointer may be NULL. */
fmx_status fmx_carve_last(fmx_ctx* ctx, fmx_carve_counts* counts, int* carved);
/* The downloads with misses.  Any array may be NULL and is then skipped. */
typedef struct fmx_voxel_arrays {
  double* xyz;
  uint64_t* scan;
  uint32_t* index;
  uint32_t* hits;
  uint32_t* misses;
} fmx_voxel_arrays;
/* fmx_dense_download that takes a voxel iff hits >= max(min_hits, 1) and, when miss_den != 0,
 * misses * miss_den <= hits * miss_num in 64-bit integers.  The two-call protocol: arrays
 * NULL, or all five of its pointers NULL, is the sizing call; otherwise *n is the capacity on
 * entry (FMX_E_SIZE if too small: nothing written) and the count on return.  misses reads 0
 * on a map that never enabled carving.  FMX_E_STATE unless the dense map is configured and
 * enabled; FMX_E_INVAL for n NULL.  fmx_dense_download is this call with misses = NULL and
 * miss_den = 0. */
fmx_status fmx_carve_download(fmx_ctx* ctx, uint32_t min_hits, uint32_t miss_num, uint32_t miss_den,
                              const fmx_voxel_arrays* arrays, uint32_t* n);
/* fmx_roll_evict and fmx_roll_drain with the struct (arrays NULL, or all five pointers NULL:
 * discard / the sizing call), with their status codes; those two are these with misses =
 * NULL.  The spill keeps misses. */
fmx_status fmx_carve_evict(fmx_ctx* ctx, const double centre[3], const uint32_t half[3],
                           const fmx_voxel_arrays* arrays, uint32_t* n);
fmx_status fmx_carve_drain(fmx_ctx* ctx, const fmx_voxel_arrays* arrays, uint32_t* n);

/* ---------------- probing the dense voxel map: lookups and first-hit ray casts ----
 * Questions about a few thousand places, answered on the device without a download
 * (DESIGN.md §Dense map, Probing).  Both calls only read: the table, the counters,
 * fmx_dense_stats, fmx_dense_last, fmx_carve_last, the spill and the estimator are as before.
 * All of it is exact, fp64 without contraction, one rounding per written operation
 * (tests/probe_ref.py restates it):
 *   filter   min_hits, miss_num, miss_den.  A stored voxel is solid iff hits >= max(min_hits, 1)
 *            and, when miss_den != 0, misses * miss_den <= hits * miss_num in 64-bit integers:
 *            fmx_carve_download's rule.  misses reads 0 on a map that never enabled carving;
 *   point    input point i (fp32 xyzw, host or device memory, n_points < 2^32) at pose34 is
 *            invalid when x, y or z is not finite or x = y = z = 0 (the integration's rule;
 *            the dense gate plays no part).  Otherwise its world point is the integration's
 *            expression and its voxel c_k = floor(w_k / voxel_width); out_of_range unless
 *            every |c_k| < 2^20 - 1, tested in fp64 before the cast;
 *   lookup   find only: home slot mix64 of the key & (slots - 1), linear probing up to the
 *            key or an empty slot;
 *   outputs  host arrays aligned with the input, index i to point i.  Any pointer may be NULL
 *            (voxels NULL: all five of its pointers NULL) and is then neither computed into
 *            nor copied.  Where no voxel is reported the five voxel fields are written as
 *            zeros; scan is the scan_idx of the integration that owns the voxel.
 * Status codes of both: FMX_E_STATE unless the dense map is configured and enabled;
 * FMX_E_INVAL for a NULL or non-finite pose, NULL points with n_points > 0 or n_points >=
 * 2^32; FMX_E_OOM, nothing written, when a per-call device buffer cannot be allocated.
 * n_points == 0 succeeds with zero counts.  The calls run after whatever integration or roll
 * is queued and return once the outputs are in.  A context that never calls them allocates
 * and launches nothing for them. */
#define FMX_PROBE_ABSENT 0        /* the voxel is not in the map; a ray: no solid voxel examined */
#define FMX_PROBE_FILTERED 1      /* present but not solid */
#define FMX_PROBE_SOLID 2         /* present and solid; a ray: it ended in this voxel */
#define FMX_PROBE_OUT_OF_RANGE 3
#define FMX_PROBE_INVALID 4
#define FMX_PROBE_NO_STEP 0xFFFFFFFFu
typedef struct fmx_probe_point_counts {
  uint32_t absent;
  uint32_t filtered;
  uint32_t solid;
  uint32_t out_of_range;
  uint32_t invalid;          /* the five sum to n */
} fmx_probe_point_counts;
typedef struct fmx_probe_ray_counts {
  uint32_t hit;
  uint32_t clear;
  uint32_t out_of_range;
  uint32_t invalid;          /* the four sum to n */
  uint64_t steps;            /* voxels examined, the hit voxel included and nothing behind it */
} fmx_probe_ray_counts;
/* One lookup per point: state[i] is one of the five values above, and for FILTERED and SOLID
 * the voxel's fields are returned. */
fmx_status fmx_probe_points(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                            const double pose34[12], uint32_t min_hits, uint32_t miss_num, uint32_t miss_den,
                            uint8_t* state, const fmx_voxel_arrays* voxels, fmx_probe_point_counts* counts);
/* One segment cast per point, from the pose's translation o to the point's world point e.
 * Invalid and out_of_range as above, the latter for the end voxel b; a = floor(o / w) by the
 * carve's rule: FMX_E_RANGE, nothing written, unless every |a_k| < 2^20 - 1.  The walk is the
 * carve's, word for word (above, "walk"): v_0 = a ... v_S = b.  Examined, in order: v_s for
 * skip <= s <= S, the end voxel included (skip: the sensor's own voxels).  The first examined
 * voxel that is present and solid ends the ray (one present but not solid is transparent):
 * state SOLID, step[i] = s, t[i] = the tau of the step that entered v_s (0.0 for s = 0; the
 * range is t |e - o|), and the voxel's fields.  Otherwise state ABSENT, and for every state
 * but SOLID step[i] = FMX_PROBE_NO_STEP and t[i] = +inf.  counts->steps is the definition's
 * number, whatever the kernel loads ahead. */
fmx_status fmx_probe_rays(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                          const double pose34[12], uint32_t min_hits, uint32_t miss_num, uint32_t miss_den,
                          uint32_t skip, uint8_t* state, uint32_t* step, double* t,
                          const fmx_voxel_arrays* voxels, fmx_probe_ray_counts* counts);

/* ---------------- loading voxels back into the dense voxel map -------------------
 * The inverse of the downloads: voxel records, as fmx_carve_download, fmx_carve_evict and
 * fmx_carve_drain hand them out, go back into the table (DESIGN.md §Dense map, Restoring).  A
 * roll's spill can return when the sensor does, a map can be saved and resumed, two contexts'
 * maps can be merged.  All arrays are host arrays of n entries; the semantics are exact and do
 * not depend on the order the device's threads run in (tests/upload_ref.py restates them):
 *   classes  entry i is invalid when a coordinate of xyz[i] is not finite, or hits is given and
 *            hits[i] == 0 (a world point of exactly (0, 0, 0) is valid: the all-zero rule
 *            belongs to sensor-frame points).  Otherwise its voxel is c_k = floor(xyz_k /
 *            voxel_width) in fp64, the integration's expression, with no pose and no gate;
 *            out_of_range unless every |c_k| < 2^20 - 1, tested in fp64 before the cast.  (A
 *            representative was stored in the voxel it fell into: a downloaded point names
 *            its own voxel again.)
 *   resident the voxel is in the table: it keeps its representative (point, scan, index) bit
 *            for bit, its hits grow by the sum of the entries' hits and its misses by the sum
 *            of their misses; every such entry counts as merged.
 *   absent   the voxel is opened and counts as added once.  Its representative is the entry
 *            with the lowest input position among the valid entries of that voxel in this
 *            call: xyz, scan and index are stored as given (any u64, any u32), hits and misses
 *            are the sums over all of them; the other entries count as merged.  Spills kept
 *            over time and concatenated in time order: the oldest owner wins.
 * Sums are modulo 2^32, as the integration's.  An uploaded voxel behaves like any other from
 * then on: integrations add to its hits, the carve may count misses on it (the upload never
 * exempts it), rolls keep or evict it, downloads and probes return scan and index as given.
 * An upload is not an integration: fmx_dense_stats' integration counter, the integration
 * numbers that the carve's `every` counts, fmx_dense_last, fmx_carve_last, the roll's centre,
 * its statistics and the spill are unchanged; fmx_dense_clear forgets uploaded voxels like
 * all others.  The capacity rule is the integration's: FMX_E_OOM, nothing launched and
 * nothing changed, unless voxels + n <= max_voxels.
 * Status codes: FMX_E_STATE unless the dense map is configured and enabled; FMX_E_INVAL for
 * in NULL, or xyz NULL with n > 0; FMX_E_STATE when misses is given and carving was never
 * enabled on this map (there is no array to hold them); FMX_E_OOM by the capacity rule or
 * when a per-call buffer cannot be allocated, FMX_E_STATE when the owner numbering (32 bits,
 * one per integration and per distinct scan value of an upload since the last clear) would
 * be exhausted: nothing changed in either case.  n == 0 succeeds with zero counts and
 * launches nothing.  The call runs after whatever integration or roll is queued and returns
 * once the counts are in.  A context that never calls it allocates and launches nothing for
 * it. */
typedef struct fmx_voxel_input {   /* fmx_voxel_arrays, read-only */
  const double* xyz;       /* 3 n, required when n > 0 */
  const uint64_t* scan;    /* NULL: 0 for every entry */
  const uint32_t* index;   /* NULL: 0 */
  const uint32_t* hits;    /* NULL: 1 */
  const uint32_t* misses;  /* NULL: 0 */
} fmx_voxel_input;
typedef struct fmx_upload_counts {
  uint32_t added;          /* new voxels */
  uint32_t merged;         /* valid entries that did not become a representative */
  uint32_t out_of_range;
  uint32_t invalid;        /* the four sum to n */
} fmx_upload_counts;
fmx_status fmx_upload_voxels(fmx_ctx* ctx, const fmx_voxel_input* in, uint32_t n,
                            fmx_upload_counts* counts /* may be NULL */);

/* ---------------- the nearest solid voxel of the dense map: radius search -------------
 * How far is the nearest surface from a point, and which voxel is it: answered on the device
 * without a download (DESIGN.md §Dense map, Nearest).  The call only reads: the table, the
 * counters, fmx_dense_stats, fmx_dense_last, fmx_carve_last, the spill and the estimator are as
 * before.  All of it is exact, fp64 without contraction, one rounding per written operation
 * (tests/nearest_ref.py restates it):
 *   point    the classes of fmx_probe_points, word for word: invalid by the integration's rule;
 *            otherwise the world point p is the integration's expression and the own voxel
 *            c_k = floor(p_k / voxel_width); out_of_range unless every |c_k| < 2^20 - 1, tested
 *            in fp64 before the cast.  The dense gate plays no part;
 *   filter   fmx_carve_download's rule, as for the probes: solid iff hits >= max(min_hits, 1)
 *            and, when miss_den != 0, misses * miss_den <= hits * miss_num in 64-bit integers.
 *            misses reads 0 on a map that never enabled carving;
 *   cube     the candidates are the cells c + d with every |d_k| <= reach.  A cell with a
 *            coordinate outside |.| < 2^20 - 1 cannot be stored and is skipped; every other is
 *            looked up find-only.  A present and solid voxel with representative q has
 *            e_k = q_k - p_k and d2 = (e_0 * e_0 + e_1 * e_1) + e_2 * e_2, and is admitted iff
 *            d2 <= max_dist2 (+inf: no limit; 0: coincident points only);
 *   winner   the admitted candidate with the smallest d2; among equal d2 the one with the
 *            smallest packed key ((c_0 + 2^20) << 42 | (c_1 + 2^20) << 21 | c_2 + 2^20) as u64;
 *   outputs  host arrays aligned with the input.  state[i] is FMX_PROBE_SOLID (found),
 *            FMX_PROBE_ABSENT (none), FMX_PROBE_OUT_OF_RANGE or FMX_PROBE_INVALID, never
 *            FMX_PROBE_FILTERED.  dist2[i] is the winner's d2, +inf for every other state.  The
 *            winner's five voxel fields are returned, zeros otherwise; scan is the scan_idx of
 *            the owner of the voxel.  Any pointer may be NULL (voxels NULL: all five of its
 *            pointers NULL) and is then neither computed into nor copied.
 * What a result certifies.  A representative lies in the cell its key names up to the one
 * rounding of floor(x / voxel_width), for an integrated and for an uploaded voxel alike, so a
 * voxel outside the cube is farther than (reach - 2^-32) * voxel_width from p: a result with
 * d2 below the square of that is the nearest solid representative of the whole map.  A call
 * with max_dist2 = r * r and reach = floor(r / voxel_width) + 1 is therefore an exact radius
 * search: the nearest solid representative within r, or none.
 * counts->lookups is the number of cells the kernel looked up, summed over the points: a
 * diagnostic for the cost model that depends on what the kernel may skip (a finished shell s >=
 * 1 ends a point's search once the best d2, or max_dist2, is below (1 - 2^-20) (s w)^2).  It is
 * at least the number of valid in-range points and at most the number of storable cube cells
 * of those points; the outputs and the four class counts are the definition's whatever is
 * skipped.
 * Status codes: FMX_E_STATE unless the dense map is configured and enabled; FMX_E_INVAL for a
 * NULL or non-finite pose, NULL points with n_points > 0, n_points >= 2^32, reach >
 * FMX_NEAREST_MAX_REACH, or a NaN or negative max_dist2; FMX_E_OOM, nothing written, when a
 * per-call buffer cannot be allocated.  n_points == 0 succeeds with zero counts and launches
 * nothing.  The call runs after whatever integration or roll is queued and returns once the
 * outputs are in.  A context that never calls it allocates and launches nothing for it. */
#define FMX_NEAREST_MAX_REACH 8
typedef struct fmx_nearest_counts {
  uint32_t found;
  uint32_t none;
  uint32_t out_of_range;
  uint32_t invalid;          /* the four sum to n */
  uint64_t lookups;          /* cells the kernel looked up: a diagnostic, see above */
} fmx_nearest_counts;
fmx_status fmx_nearest_voxels(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                              const double pose34[12], uint32_t min_hits, uint32_t miss_num, uint32_t miss_den,
                              uint32_t reach, double max_dist2, uint8_t* state, double* dist2,
                              const fmx_voxel_arrays* voxels, fmx_nearest_counts* counts);

/* ---------------- aligning a scan to the dense map: registration on the device ---------
 * Where is the sensor in a map that was built, or loaded back: the point-to-point
 * Gauss-Newton registration of a scan against the map's solid representatives, the search and
 * the linearization fused into one launch per iteration that returns 29 doubles and five
 * counts, nothing per point (DESIGN.md §Dense map, Aligning; tests/align_ref.py restates it).
 * Both calls only read: the table, the counters, fmx_dense_stats, fmx_dense_last,
 * fmx_carve_last, the roll state, the spill and the estimator are as before, and
 * fmx_current_pose is untouched: the alignment does not feed the estimator.
 *   points   point i with i % stride != 0 (stride 0 reads 1) is skipped: neither classified nor
 *            searched.  Every other point is classified and searched exactly as
 *            fmx_nearest_voxels does it (the block above: point, filter, cube, winner), with
 *            params' min_hits, miss_num, miss_den, reach and max_dist2 in their places there;
 *   rows     a found point has its sensor-frame point p (the fp32 input widened to double), its
 *            world point w (the integration's expression) and the winner's representative q,
 *            and contributes three rows a = 0, 1, 2, R_a being row a of the pose's rotation:
 *              r_a = w_a - q_a
 *              H_a = [R_a2 p_1 - R_a1 p_2, R_a0 p_2 - R_a2 p_0, R_a1 p_0 - R_a0 p_1,
 *                     R_a0, R_a1, R_a2]
 *            (tangent [w; v], right perturbation: the point-to-point factor of
 *            fmx_linearize with X(i) the identity and p_i = q);
 *   output   with inv = 1 / sigma and v = [H_a * inv, -r_a * inv], out[0..27] is the packed
 *            upper 7 x 7 of the sum of v v^T over all rows, packed as fmx_linearize_matched
 *            packs it (index r * 7 - r (r - 1) / 2 + (q - r)), and out[28] = 0.5 * the sum of
 *            (r_a * inv)^2.  Per-point terms are fp64 without contraction;
 *   order    the order of the sum is the kernel's, fixed by n_points, stride and the launch
 *            grid alone and not by the order the threads run in: two calls with the same
 *            arguments on the same map return the same 29 bit patterns, from a host and from
 *            a device pointer alike.  The class counts are the definition's exactly;
 *            counts->lookups is fmx_nearest_counts' diagnostic, under its bounds.
 * fmx_align_dense is fmx_register_points' loop on that system.  From T = pose_init, while
 * iters < max_iters: evaluate the system at T (++iters), solve H dx = g by Cholesky, T = T *
 * Exp(dx), stop once ||dx|| < threshold.  The scan is staged to the device once per call; an
 * iteration is one memset of the counters, one launch, one wait on a completion word and the
 * host's 6 x 6 solve.  max_iters == 0 returns pose_init with iters = 0.
 * Status codes: FMX_E_STATE unless the dense map is configured and enabled, and, pose_out left
 * unwritten, when a system is singular (too few found points); FMX_E_INVAL for NULL params,
 * out, pose or pose_out, a non-finite pose, NULL points with n_points > 0, n_points >= 2^32,
 * reach > FMX_NEAREST_MAX_REACH, a NaN or negative max_dist2, a sigma that is not finite and
 * positive, a NaN or negative threshold; FMX_E_OOM, nothing written, when a per-call buffer
 * cannot be allocated.  fmx_align_system with n_points == 0 succeeds with an all-zero system
 * and launches nothing.  A context that calls neither allocates and launches nothing for
 * them. */
typedef struct fmx_align_params {
  uint32_t min_hits, miss_num, miss_den;  /* fmx_carve_download's filter */
  uint32_t reach;                         /* <= FMX_NEAREST_MAX_REACH */
  double max_dist2;                       /* fmx_nearest_voxels' rule */
  double sigma;                           /* > 0, finite */
  uint32_t stride;                        /* use points with i % stride == 0; 0 = 1 */
} fmx_align_params;
typedef struct fmx_align_counts {
  uint32_t found, none, out_of_range, invalid, skipped;  /* the five sum to n */
  uint64_t lookups;                                      /* diagnostic, as fmx_nearest_counts */
} fmx_align_counts;
fmx_status fmx_align_system(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                            const double pose34[12], const fmx_align_params* params, double out[29],
                            fmx_align_counts* counts /* may be NULL */);
typedef struct fmx_align_result {
  uint32_t iters;          /* systems evaluated */
  int32_t converged;       /* 1 iff the last step's norm < threshold */
  double last_step;        /* ||dx|| of the last step, 0 when iters == 0 */
  double error;            /* out[28] of the last system evaluated */
  fmx_align_counts counts; /* of the last system evaluated */
} fmx_align_result;
fmx_status fmx_align_dense(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                           const double pose_init34[12], const fmx_align_params* params, uint32_t max_iters,
                           double threshold, double pose_out34[12], fmx_align_result* result /* may be NULL */);

/* ---------------- surface normals of the dense map: one snapshot per build ---------------
 * A per-voxel normal field computed on the device from the map's solid representatives, kept
 * beside the table, one record per table slot: the normal (3 floats) and the flatness (1 float)
 * in one 16-byte word, and the support (uint32): 20 bytes per slot on top of the table's 44 (52
 * with carving), allocated at the first fmx_normals_build (DESIGN.md §Dense map, Normals;
 * tests/normals_ref.py restates it).  The build only reads the table.
 * Semantics, fp64 without contraction.  For every stored voxel with representative q0:
 *   filtered  not solid under fmx_carve_download's rule with params' min_hits, miss_num,
 *             miss_den: support 0, no normal;
 *   support   otherwise the neighbours are the present and solid voxels of the cells within
 *             `reach` of the voxel's own cell (the cell its key names), the own cell included,
 *             cells that cannot be stored skipped as in fmx_nearest_voxels.  A neighbour with
 *             representative q has e = q - q0 and d2 = (e_0 e_0 + e_1 e_1) + e_2 e_2 and is
 *             admitted iff d2 <= max_dist2 (+inf: the whole cube); support = k, the number
 *             admitted (k >= 1: the voxel admits itself);
 *   moments   S1 = sum e, S2 = sum e e^T (six entries), m = S1 / k, C_ab = S2_ab / k - m_a m_b;
 *             l0 <= l1 <= l2 the eigenvalues of C (cyclic Jacobi in fp64), a negative l0 read
 *             as 0; n the unit eigenvector of l0, its sign such that the component of largest
 *             magnitude is positive (the lowest axis among equal magnitudes: nothing in the
 *             table knows where the sensor was); flatness = l0 / l1, +inf when l1 <= 0;
 *   class     sparse when k < max(min_support, 3); else oriented iff l1 > 0 and l0 <=
 *             max_flatness * l1; else flat_rejected;
 *   stored    n rounded once to fp32, all zeros unless oriented; flatness as fp32 (0 for a
 *             filtered voxel); support.
 * The order of each voxel's sums is the kernel's (the cube's cells in the fixed order of the
 * offset list, one lane per voxel), not the order the threads run in: two builds of the same
 * table with the same parameters store the same bits.  counts->lookups is the number of cells
 * looked up, a diagnostic as fmx_nearest_counts'.  One launch on the context stream; the call
 * returns once the counts are in.  An empty map launches nothing and gives zero counts.
 * Staleness.  The snapshot is indexed by slot: it is current from a successful build until the
 * next call that changed, or may have changed, the table: a successful fmx_dense_integrate or
 * register-path integration (with or without its carve), fmx_carve_rays, fmx_upload_voxels with
 * n > 0, any roll that evicts, fmx_dense_clear, and fmx_dense_configure, which also drops the
 * arrays.  fmx_normals_stats gives {built, current, voxels at the build, oriented at the
 * build}, all 0 when never built, FMX_OK on any context.
 * fmx_normals_download follows fmx_carve_download's two-call protocol (all pointers NULL: *n
 * receives the size; otherwise *n is the capacity on entry, FMX_E_SIZE with nothing written if
 * too small, and the count on return): the voxels that were solid under the build's filter, or
 * with oriented_only != 0 only the oriented ones, in no particular order; normal takes 3
 * floats per voxel; any pointer may be NULL.
 * Status codes: FMX_E_STATE unless the dense map is configured and enabled, and, for the
 * download, unless the snapshot is current; FMX_E_INVAL for NULL params or counts' pointer
 * where required, reach 0 (the own cell alone supports nothing) or > FMX_NEAREST_MAX_REACH, a
 * NaN or negative max_dist2, a max_flatness that is not finite and in [0, 1]; FMX_E_OOM when an
 * array cannot be allocated (a snapshot that was current stays so). */
typedef struct fmx_normals_params {
  uint32_t min_hits, miss_num, miss_den;  /* fmx_carve_download's filter */
  uint32_t reach;                         /* 1 .. FMX_NEAREST_MAX_REACH */
  double max_dist2;                       /* fmx_nearest_voxels' rule */
  uint32_t min_support;                   /* values below 3 read as 3 */
  double max_flatness;                    /* in [0, 1] */
} fmx_normals_params;
typedef struct fmx_normals_counts {
  uint32_t oriented, flat_rejected, sparse, filtered;  /* the four sum to the map's voxels */
  uint64_t lookups;                                    /* diagnostic, as fmx_nearest_counts */
} fmx_normals_counts;
fmx_status fmx_normals_build(fmx_ctx* ctx, const fmx_normals_params* params, fmx_normals_counts* counts /* may be NULL */);
fmx_status fmx_normals_stats(fmx_ctx* ctx, uint64_t out[4]);
fmx_status fmx_normals_download(fmx_ctx* ctx, int oriented_only, const fmx_voxel_arrays* arrays, float* normal,
                                float* flatness, uint32_t* support, uint32_t* n);

/* ---------------- point-to-plane alignment against the dense map's normals ---------------
 * fmx_align_system / fmx_align_dense with the point-to-plane residual (DESIGN.md §Dense map,
 * Plane alignment; tests/plane_ref.py restates it).  Skipping, classifying and searching are
 * fmx_align_system's, word for word: the winner is the nearest solid representative, normals
 * play no part in the search.  Both calls only read.
 *   unoriented  a found point whose winner's slot holds no normal (not oriented at the build)
 *               is counted here, not under found, and contributes nothing;
 *   row         a found point with sensor-frame point p, world point w, winner q and normal n
 *               (the stored fp32 widened) contributes one row, the plane factor of
 *               fmx_linearize with X(i) the identity, p_i = q, n_i = n, p_j = p:
 *                 r = (n_0 (w_0 - q_0) + n_1 (w_1 - q_1)) + n_2 (w_2 - q_2)
 *                 H = [m_2 p_1 - m_1 p_2, m_0 p_2 - m_2 p_0, m_1 p_0 - m_0 p_1, m_0, m_1, m_2]
 *               with m = R^T n;
 *   output      whitening, packing, out[28], the fixed order of the sums and the bit-for-bit
 *               repeatability are fmx_align_system's.  The system does not depend on the sign
 *               of n.
 * fmx_plane_align is fmx_align_dense's loop over this system; a singular system (e.g. a scan
 * that sees one plane only) is FMX_E_STATE with pose_out unwritten.
 * Status codes: fmx_align_system's / fmx_align_dense's, and FMX_E_STATE unless the normal
 * snapshot is current (fmx_normals_build). */
typedef struct fmx_plane_counts {
  uint32_t found, none, out_of_range, invalid, skipped, unoriented;  /* the six sum to n */
  uint64_t lookups;                                                  /* diagnostic, as fmx_nearest_counts */
} fmx_plane_counts;
fmx_status fmx_plane_system(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                            const double pose34[12], const fmx_align_params* params, double out[29],
                            fmx_plane_counts* counts /* may be NULL */);
typedef struct fmx_plane_result {
  uint32_t iters;          /* systems evaluated */
  int32_t converged;       /* 1 iff the last step's norm < threshold */
  double last_step;        /* ||dx|| of the last step, 0 when iters == 0 */
  double error;            /* out[28] of the last system evaluated */
  fmx_plane_counts counts; /* of the last system evaluated */
} fmx_plane_result;
fmx_status fmx_plane_align(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                           const double pose_init34[12], const fmx_align_params* params, uint32_t max_iters,
                           double threshold, double pose_out34[12], fmx_plane_result* result /* may be NULL */);

/* ---------------- scoring many candidate poses of a scan against the dense map ------------
 * Where could the sensor be when no guess lies inside the search radius (a map loaded back, a
 * lost tracker): one scan, staged once, judged at n_poses candidate poses in one call, one
 * 32-byte record per pose and nothing per point (DESIGN.md §Dense map, Scoring;
 * tests/score_ref.py restates it).  The call only reads: the table, the counters, the normal
 * snapshot's `current` flag, the roll state, the spill, fmx_dense_stats, fmx_dense_last,
 * fmx_carve_last, the estimator and fmx_current_pose are as before.
 *   points   for every pose k independently, point i with i % stride != 0 (stride 0 reads 1) is
 *            skipped: neither classified nor searched.  Every other point is classified and
 *            searched exactly as fmx_nearest_voxels does it at poses34[k] (its block above:
 *            point, filter, cube, winner), with params' min_hits, miss_num, miss_den, reach and
 *            max_dist2 in their places there.  sigma is validated as fmx_align_system validates
 *            it and enters nothing;
 *   counts   found, none, out_of_range and invalid are that definition's counts, exactly; the
 *            four sum to ceil(n_points / stride);
 *   sum_d2   the sum of the winners' d2 over the found points, each d2 the very bit pattern
 *            fmx_nearest_voxels would report; 0.0 exactly when found == 0;
 *   order    the order of the sum is fixed by n_points, stride and constants of the build
 *            alone (fmx_score_plan reports them): the kept points in tiles, a tile's waves by a
 *            fixed butterfly and then in wave order, a pose's tiles by a fixed lane-to-tile
 *            assignment and the same butterfly.  It does not depend on the order the threads
 *            run in, on n_poses, or on a pose's place in the list: scores[k] is a function of
 *            the points, the stride, the params, the map and pose k only.  A permuted pose list
 *            gives the permuted records bit for bit, a call with that one pose the same 32
 *            bytes, a host and a device point pointer the same bits: the call splits a long
 *            list into chunks without anyone seeing it;
 *   lookups  fmx_nearest_counts' diagnostic, under its bounds.
 * The scan is staged once per call, the poses once per chunk; a chunk is two launches (the
 * (pose, tile) partial records, then one wave per pose summing its tiles) and the records'
 * copy out.  The call runs after whatever integration or roll is queued and returns once
 * scores is written.  A context that never calls it allocates and launches nothing for it.
 * Status codes: FMX_E_STATE unless the dense map is configured and enabled; FMX_E_INVAL for
 * NULL params, NULL poses34 or scores with n_poses > 0, any non-finite pose entry (scores is
 * untouched then), n_poses > FMX_SCORE_MAX_POSES, and every fmx_align_system case on points,
 * n_points, reach, max_dist2 and sigma; FMX_E_OOM, nothing written, when a per-call buffer
 * cannot be allocated.  n_poses == 0 succeeds, launches nothing and writes nothing; n_points ==
 * 0 with n_poses > 0 succeeds, launches nothing and writes all-zero records.
 * fmx_score_plan (host only: no context, no device, like fmx_pair_sort_plan) reports the tiling
 * and the chunking of such a call: out = {the kept points, the points per tile, the tiles per
 * pose, the poses per chunk (min(16384, what keeps the partial records within 32 MiB), at least
 * 1), the chunks of this call (0 when nothing is launched), the grid's cap in blocks}.
 * FMX_E_INVAL for NULL out, n_poses > FMX_SCORE_MAX_POSES, or n_points >= 2^32. */
#define FMX_SCORE_MAX_POSES 65536
typedef struct fmx_pose_score {
  uint32_t found, none, out_of_range, invalid; /* the four sum to ceil(n_points / stride) */
  double sum_d2;                               /* sum of the winners' d2 over the found points */
  uint64_t lookups;                            /* diagnostic, as fmx_nearest_counts' */
} fmx_pose_score;
fmx_status fmx_score_poses(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                           const double* poses34 /* host, n_poses x 12 */, uint32_t n_poses,
                           const fmx_align_params* params, fmx_pose_score* scores /* host, n_poses */);
fmx_status fmx_score_plan(uint64_t n_points, uint32_t stride, uint32_t n_poses, uint32_t out[6]);

/* ---------------- refining many candidate poses at once: batched alignment systems --------
 * The batched form of the alignment itself: the 7 x 7 Gauss-Newton system of one staged scan at
 * n_poses poses in one call, point-to-point (plane == 0: fmx_align_system's) or point-to-plane
 * (plane != 0: fmx_plane_system's), one 264-byte record per pose and nothing per point, and on
 * top of it a Gauss-Newton loop that advances all poses in lockstep (DESIGN.md §Dense map,
 * Refining; tests/refine_ref.py restates it).  Both calls only read: the table, the counters,
 * the normal snapshot's `current` flag, the roll state, the spill, fmx_dense_stats,
 * fmx_dense_last, fmx_carve_last, the estimator and fmx_current_pose are as before.
 * fmx_refine_systems:
 *   points   for every pose k independently, the points with i % stride == 0 (stride 0 reads 1)
 *            are classified and searched exactly as fmx_align_system, or with plane != 0
 *            fmx_plane_system, does it at poses34[k], and each found point contributes the very rows
 *            it contributes there: every per-point term has the same bits;
 *   counts   found, none, out_of_range, invalid and, in the plane form, unoriented (0 in the
 *            point form) are that definition's counts, exactly; they sum to ceil(n_points /
 *            stride).  `skipped` is the same for every pose and is not repeated per record;
 *            reserved is 0; lookups is fmx_nearest_counts' diagnostic;
 *   S        S[0..27] is the packed upper 7 x 7 of the sum of the rows' v v^T and S[28] =
 *            0.5 * S[27], as fmx_align_system's out.  A pose at which nothing is found has S
 *            all +0.0;
 *   order    the order of each of the 28 sums is fixed by n_points, stride and constants of the
 *            build alone (fmx_refine_plan reports them): a lane's kept points of a tile in
 *            index order, a wave by a fixed reduce-scatter, a tile's waves in wave order, a
 *            pose's tiles in an order fixed by their number.  It does not depend on the order the threads run in, on
 *            n_poses, or on a pose's place in the list: out[k] is a function of the points, the
 *            stride, the params, plane, the map (and the normal snapshot) and pose k only.  A
 *            permuted pose list gives the permuted records byte for byte, a call with that one
 *            pose the same 264 bytes, a host and a device point pointer the same bytes: the
 *            call splits a long list into chunks without anyone seeing it.  The order is not
 *            fmx_align_system's, whose order depends on its launch grid: against that call at
 *            the same pose the sums agree to rounding, not bit for bit; the counts and lookups
 *            are equal.
 * fmx_refine_poses runs fmx_align_dense's recurrence for every pose k on its own records.  From
 * T = poses_init34[k], while iters < max_iters: take its system at T (++iters), solve H dx = g
 * by Cholesky, T = T * Exp(dx), stop once ||dx|| < threshold.  All poses that are still running
 * are evaluated together, one batched evaluation per round, in list order; because a record
 * depends on its own pose alone, poses_out34[k] and results[k] are byte for byte what a call
 * with that one pose returns.  A pose whose system is singular (too few found points) leaves the
 * loop with singular = 1 and converged = 0, its iters counting the singular evaluation, error
 * and the counts those of the singular system, last_step that of the last step it took (0 when
 * it took none), and poses_out34[k] = poses_init34[k] bit for bit; the call still returns
 * FMX_OK: one bad candidate does not fail the others.  max_iters == 0 returns the initial poses
 * with iters = 0.  The scan is staged once per call; a round stages the active poses, runs two
 * launches per chunk (the (pose, tile) partial records, then one block per pose summing its
 * tiles), copies the records out and waits once; the 6 x 6 solves are the host's.
 * Status codes: FMX_E_STATE unless the dense map is configured and enabled, and, with plane !=
 * 0, unless the normal snapshot is current; FMX_E_INVAL, the outputs untouched, for NULL params,
 * NULL poses or outputs (results may be NULL) with n_poses > 0, any non-finite pose entry,
 * n_poses > FMX_REFINE_MAX_POSES, every fmx_align_system case on points, n_points, reach,
 * max_dist2 and sigma, and for the loop a NaN or negative threshold; FMX_E_OOM, nothing
 * written, when a per-call buffer cannot be had.  n_poses == 0 succeeds and writes nothing;
 * n_points == 0 with n_poses > 0 succeeds, launches nothing and writes all-zero systems (in the
 * loop every pose is then singular at iteration 1).  A context that never calls these
 * functions allocates and launches nothing for them.
 * fmx_refine_plan (host only: no context, no device, like fmx_score_plan) reports the tiling
 * and the chunking of such a call: out = {the kept points, the kept points per tile, the tiles
 * per pose, the poses per chunk (min(16384, what keeps the partial records within 32 MiB), at
 * least 1), the chunks of this call (0 when nothing is launched), the grid's cap in blocks}.
 * FMX_E_INVAL for NULL out, n_poses > FMX_REFINE_MAX_POSES, or n_points >= 2^32. */
#define FMX_REFINE_MAX_POSES 65536
typedef struct fmx_refine_system { /* 264 bytes */
  double S[29];                    /* packed upper 7 x 7 and the error, as fmx_align_system's out */
  uint32_t found, none, out_of_range, invalid, unoriented, reserved; /* they sum to ceil(n_points / stride) */
  uint64_t lookups;                /* diagnostic, as fmx_nearest_counts' */
} fmx_refine_system;
fmx_status fmx_refine_systems(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                              const double* poses34 /* host, n_poses x 12 */, uint32_t n_poses,
                              const fmx_align_params* params, int plane, fmx_refine_system* out /* host, n_poses */);
typedef struct fmx_refine_result {
  uint32_t iters;     /* systems evaluated */
  int32_t converged;  /* 1 iff the last step's norm < threshold */
  int32_t singular;   /* 1 iff the loop ended on a singular system */
  uint32_t reserved;  /* 0 */
  double last_step;   /* ||dx|| of the last step taken, 0 when none was */
  double error;       /* S[28] of the last system evaluated */
  uint32_t found, none, out_of_range, invalid, unoriented, reserved2; /* of the last system evaluated */
  uint64_t lookups;
} fmx_refine_result;
fmx_status fmx_refine_poses(fmx_ctx* ctx, const float* xyzw, size_t n_points, int src_on_device,
                            const double* poses_init34 /* host, n_poses x 12 */, uint32_t n_poses,
                            const fmx_align_params* params, int plane, uint32_t max_iters, double threshold,
                            double* poses_out34 /* host, n_poses x 12 */, fmx_refine_result* results /* may be NULL */);
fmx_status fmx_refine_plan(uint64_t n_points, uint32_t stride, uint32_t n_poses, uint32_t out[6]);

/* Estimator::current_lidar_estimate (form/form.hpp:79).  With deskewing on: the sensor
 * pose at the middle of the last registered sweep. */
fmx_status fmx_current_pose(fmx_ctx* ctx, double pose34[12]);
/* FORM::map() (python/bindings.cpp:96-119): KeypointMap::to_voxel_map of both feature
 * types (map.tpp:128-146) at the current window estimates, voxel width voxel_width
 * (the binding passes min_dist_map, bindings.cpp:100), every voxel's points in turn —
 * world frame, planar: 6 doubles (x, y, z, nx, ny, nz), point: 3 doubles, plus the
 * scan id of each (the binding ships it as the point's column, bindings.cpp:31-41).
 * Voxel order is unspecified (the reference iterates a robin_map); inside a voxel,
 * push_back order (scans ascending, then keypoint order).  Two calls: with NULL
 * buffers *n_planar / *n_point receive the sizes; with buffers they are the
 * capacities on entry (FMX_E_SIZE if too small) and the counts on return.  Needs a
 * registered scan (FMX_E_STATE otherwise). */
fmx_status fmx_map_download(fmx_ctx* ctx, double voxel_width, double* planar, uint64_t* planar_scan,
                            uint32_t* n_planar, double* point, uint64_t* point_scan, uint32_t* n_point);

/* Statistics of the last register_scan, the first n of: {icp_iters, lm_iters,
 * matched_planar, matched_point, map_planar, map_point, linearizations, map_scans,
 * host_waits (host<->device round trips: waits on a completion word or the stream),
 * spec_matches (speculative matches launched at LM-trial poses), spec_hits (ICP
 * iterations that used one instead of matching), spec_map (1 when the scan's map was
 * the one built speculatively during the previous scan's final LM, 0 when built at
 * the start of this scan), pipelined (1 when the scan's features were extracted
 * during the previous registration, fmx_next_scan), window_poses (poses in the
 * smoother's window after the scan: the host LM's system is 6 x window_poses)},
 * followed by five counts since fmx_create that every entry point advances, the seam API's
 * fmx_keypoints_add and fmx_map_insert included: {pool_compactions_planar,
 * pool_compactions_point (the keypoint pool moved its live scans to a fresh buffer),
 * win_compactions (the smoothing-mode window store moved its live rows to its other
 * arena), win_growths_plane, win_growths_point (... into a larger one)};
 * entries past the known ones read 0. */
fmx_status fmx_last_stats(fmx_ctx* ctx, uint64_t* stats, int n);
/* Work of the last fmx_match (counted by the kernel, available while profiling is
 * enabled): queries, hash probes, candidate records distance-tested. */
fmx_status fmx_match_work(fmx_ctx* ctx, double work[3]);
/* The warm certificate of the last fmx_match (no profiling needed).  A match on the same
 * map and query set as the previous one starts warm; a warm query whose previous nearest
 * record provably stays nearest after the pose step (it kept its cell, and every other
 * record was farther than that record by more than twice the step) skips the search —
 * the result is identical to a search (VoxelMap::find_closest, map.tpp:70-91).
 * counts[0] = certified queries, counts[1] = warm queries (either may be 0);
 * certified (may be NULL): per query (planar then point) 1 if it was certified. */
fmx_status fmx_match_cert(fmx_ctx* ctx, uint64_t counts[2], uint8_t* certified);

/* ---------------- profiling (bench.py roofline) ----------------------------
 * When enabled, each kernel launch is bracketed by HIP events on the context
 * stream.  fmx_profile_read fills, for kernel id k < n: total ms, launches and
 * algorithmic bytes accumulated since the last reset. */
fmx_status fmx_profile_enable(fmx_ctx* ctx, int on);
fmx_status fmx_profile_reset(fmx_ctx* ctx);
int fmx_profile_count(void);
const char* fmx_profile_name(int k);
fmx_status fmx_profile_read(fmx_ctx* ctx, double* ms, uint64_t* launches, double* bytes, int n);
/* Match work of the profiled match launches since the last reset, cold (the first match
 * on a map / query set) then warm: {launches, queries, probes, candidates, certified
 * queries, warm queries} each (fmx_match_cert's counts, summed). */
fmx_status fmx_profile_match_work(fmx_ctx* ctx, double out[12]);

/* Wait for all of the context's device work (its stream and the side streams of the
 * map build and the pipelined extraction). */
fmx_status fmx_sync(fmx_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* FMX_FMX_H_ */
