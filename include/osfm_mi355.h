/*
 * osfm_mi355.h -- C ABI of libosfm_mi355.so, the MI355X-native drop-in for OpenSfM's
 * feature-matching + bundle-adjustment hot path.
 *
 * Every entry point is plain C: pointers + sizes, int status return (0 = OK, <0 = error, text via
 * osfm_last_error()), no exceptions, no torch types.  Host pointers unless a name says "dev".
 * The library never retains a caller pointer past the call; device memory is owned by the opaque
 * handles below.  Each entry point cites the reference interface it replaces.
 *
 * Index conventions follow the reference: a match is (feature idx in image 1, feature idx in
 * image 2) after the swap done at opensfm/matching.py:697,717-718; keypoints are normalized image
 * coordinates (opensfm/features.py:324-331); poses are angle-axis camera->world rotation + camera
 * ORIGIN (opensfm/src/bundle/data/pose.h:34-43).
 */
#ifndef OSFM_MI355_H
#define OSFM_MI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSFM_OK 0
#define OSFM_E_INVALID (-1)     /* bad argument (size mismatch, null pointer, ...) */
#define OSFM_E_HIP (-2)         /* HIP runtime error (see osfm_last_error) */
#define OSFM_E_UNSUPPORTED (-3) /* input outside the implemented domain */
#define OSFM_E_NOMEM (-4)
#define OSFM_E_NUMERIC (-5) /* NaN/Inf in results: reference throws (ba_helpers.cc:780-814) */

#define OSFM_DESC_DIM 128
#define OSFM_MAX_FEATURES 16000 /* per image (feature_min_frames_panorama, config.py:31): the matcher keeps 6 B of LDS per feature
                                   (160 KiB at 16000); the RANSAC kernel stages its correspondences in LDS up to ~9000 and in HBM above */

typedef struct osfm_ctx osfm_ctx;     /* one per process/GPU: device, streams, scratch */
typedef struct osfm_store osfm_store; /* device-resident descriptor + keypoint store */

/* Thread-local text of the last error raised on the calling thread. */
const char *osfm_last_error(void);
/* Library version string and the gfx arch the kernels were compiled for. */
const char *osfm_version(void);

int osfm_ctx_create(int device, osfm_ctx **out);
void osfm_ctx_destroy(osfm_ctx *ctx);
/* Device the context is bound to and its CU count (0 on error). */
int osfm_ctx_device(const osfm_ctx *ctx);
int osfm_ctx_num_cus(const osfm_ctx *ctx);
/* The context keeps the device blocks of its calls (the matcher's chunk buffers, the slabs a bundle adjustment sub-allocates its arrays
 * from; up to 24 GiB) cached between calls.  Waits for the device,
 * frees every cached block and returns the bytes released; the library calls it itself before it reports OSFM_E_NOMEM. */
int64_t osfm_ctx_trim_pool(osfm_ctx *ctx);

/* ------------------------------------------------------------------------------------------
 * Descriptor store.  Replaces FeatureLoader.load_all_data (opensfm/feature_loading.py:106-173):
 * instead of an LRU of per-image npz loads, all images' masked features live in HBM.
 * counts[n_images] = features per image (0..OSFM_MAX_FEATURES).
 * desc: sum(counts) x 128; float32 or uint8.  Integer-valued in [0,255] (HAHOG / SIFT uchar round trip, features.py:526-534):
 *       exact int8 matrix path.  Any other finite float32 values (root-SIFT with feature_root, features.py:292-298): the store
 *       also keeps the float rows and an 8-bit quantisation; the same kernel decides with rigorous error bounds and evaluates
 *       the undecided queries in float32 exactly as cv2 accumulates (results identical to cv2's float arithmetic as the oracle
 *       restates it).  Non-finite values: OSFM_E_INVALID.
 * pts:  sum(counts) x 2 float64 normalized image coordinates (features_data.points[:, :2]).
 * ------------------------------------------------------------------------------------------ */
int osfm_store_create(osfm_ctx *ctx, int n_images, const int32_t *counts, osfm_store **out);
int osfm_store_upload_f32(osfm_store *s, const float *desc, const double *pts);
int osfm_store_upload_u8(osfm_store *s, const uint8_t *desc, const double *pts);
/* Binary descriptors -- uint8 bit strings (AKAZE MLDB: 61 bytes, ORB: 32 bytes; width_bytes 1..64).  match_brute_force hands uint8
 * arrays to cv2's "BruteForce-Hamming" matcher (opensfm/matching.py:737-740): integer Hamming distances, the same K = 2 insertion and
 * Lowe's test on float32(int).  Instead of osfm_store_upload_f32/_u8; the store then runs osfm_match_pairs / _calibrated on the
 * Hamming kernel (VALU popcount), gates and robust stage unchanged.  Not with OSFM_MATCH_SQUARED_RATIO, guided matching or a
 * segmentation column (OSFM_E_UNSUPPORTED). */
int osfm_store_upload_binary(osfm_store *s, const uint8_t *desc, int width_bytes, const double *pts);
/* matching_use_segmentation (opensfm/feature_loading.py:118-155, matching.py:281,356): the reference appends a 129th column to the
 * HAHOG uchar descriptors, SEGMENTATION_IN_DESCRIPTOR_MULT (35) x the feature's segmentation label.  column129: sum(counts) floats,
 * that column (already multiplied).  A store that has one is matched with d^2 = d^2_128 + (c1 - c2)^2, added in float32 exactly where
 * cv2's normL2Sqr_ adds a trailing element; such stores run on the exact (VALU) kernel, not on the int8 matrix path.
 * Integer-valued stores only (the reference raises for anything but HAHOG uchar): OSFM_E_UNSUPPORTED otherwise. */
int osfm_store_set_segmentation(osfm_store *s, const float *column129);
void osfm_store_destroy(osfm_store *s);
int64_t osfm_store_bytes(const osfm_store *s); /* device bytes held */

typedef struct {
  double lowes_ratio;                /* config["lowes_ratio"], 0.8            (config.py:97)  */
  int32_t symmetric;                 /* config["symmetric_matching"]           (config.py:101) */
  int32_t robust;                    /* 1: run the geometric stage (matching.py:599-603)        */
  int32_t robust_matching_min_match; /* 20                                     (config.py:195) */
  double robust_matching_threshold;  /* 0.004                                  (config.py:191) */
  double ransac_confidence;          /* 0.9999 (matching.py:795)                               */
  int32_t ransac_max_iters;          /* 1000 (cv2.findFundamentalMat default)                  */
  int32_t flags;                     /* OSFM_MATCH_* bits below                                 */
} osfm_match_params;
#define OSFM_MATCH_EXACT_KERNEL 1  /* cross-check: run every pair on the exact VALU kernel (float keys, no MFMA; float stores:
                                      the exact float32 kernel)                                                             */
#define OSFM_MATCH_SQUARED_RATIO 2 /* matcher_type FLANN semantics on an EXACT 2-NN search: match_flann[_symmetric]
                                      (matching.py:683-720) keeps d0 < float32(lowes_ratio^2) * d1 on SQUARED float32
                                      distances; one-way matching then queries with the pair's SECOND image against the
                                      first (match_flann(index1, f2)) and lists the matches in query order.  The
                                      reference's own index (cv2.flann_Index, KMEANS, checks=20, features.py:638-674) is
                                      approximate and randomised; this is its exact limit (checks -> infinity). */
#define OSFM_MATCH_KEEP_DEVICE 4   /* the result keeps its match rows in HBM (osfm_result_dev_ptrs) instead of copying them to the
                                      host chunk by chunk: the exchange step of the multi-GPU path (all-gather of the match graph,
                                      the fan-in of matching.py:83-98 across ranks) reads them from there.  osfm_result_fetch still
                                      works (one D2H copy on demand).                                                           */

#define OSFM_MATCH_SWEEP_32X32 8   /* cross-check: the integer store's fused kernel on v_mfma_i32_32x32x32_i8 (the kernel the float
                                      store runs) instead of the default v_mfma_i32_16x16x64_i8 sweep; same results             */

void osfm_match_params_default(osfm_match_params *p);

typedef struct {
  double ms_total;         /* stream time of the whole call (HIP events)                 */
  double ms_match_kernel;  /* sum of fused distance/top-2/ratio/mutual kernel launches   */
  double ms_ransac_kernel; /* sum of RANSAC kernel launches                              */
  int64_t match_launches;
  int64_t pairs;           /* pairs processed                                            */
  int64_t pairs_exact_path; /* pairs re-run on the exact float-key kernel (d^2 >= 2^22); float store: pairs in which at least
                               one query went through the float32 evaluation                */
  int64_t pairs_ransac;    /* calibrated branch: pairs that reached the geometric stage  */
  int64_t ransac_model_points; /* F-RANSAC: sum over pairs of (models scored) x (correspondences): the work its roofline counts */
} osfm_match_timings;

/* Opaque result of a batched run: per pair a count and a list of (i, j) int32. */
typedef struct osfm_match_result osfm_match_result;

/*
 * Batched pair matching: replaces the body of match_images_with_pairs
 * (opensfm/matching.py:63-98; per pair: match(), matching.py:563-634, BRUTEFORCE symmetric +
 * robust_match_fundamental).  pairs: n_pairs x 2 image indices into the store.
 */
int osfm_match_pairs(osfm_ctx *ctx, const osfm_store *store, const int32_t *pairs, int64_t n_pairs,
                     const osfm_match_params *params, osfm_match_result **out,
                     osfm_match_timings *timings_or_null);
int64_t osfm_result_num_pairs(const osfm_match_result *r);
int64_t osfm_result_total_matches(const osfm_match_result *r);
/* counts[n_pairs]; matches[total x 2] concatenated in pair order, each pair sorted by (i, j). */
int osfm_result_fetch(const osfm_match_result *r, int32_t *counts, int32_t *matches);
/* The same two arrays where the call left them in host memory -- no copy: valid until osfm_result_destroy, not to be written through.
 * (What a binding wraps as its array type: the reference's match_images hands out per-pair numpy arrays, matching.py:563-634; the
 * Python layer here views these buffers and destroys the result when the last view goes.)  OSFM_E_INVALID for a result kept on the
 * device (OSFM_MATCH_KEEP_DEVICE: use osfm_result_fetch or osfm_result_dev_ptrs). */
int osfm_result_host_ptrs(const osfm_match_result *r, const int32_t **counts, const int32_t **matches);
/* Results of a call made with OSFM_MATCH_KEEP_DEVICE: device pointers (on osfm_result_device) to counts[n_pairs] and to the
 * concatenated matches[total x 2], valid until osfm_result_destroy; every kernel that wrote them has completed when the matching
 * call returns.  OSFM_E_INVALID for a result that was not kept on the device. */
int osfm_result_dev_ptrs(const osfm_match_result *r, const int32_t **d_counts, const int32_t **d_matches);
int osfm_result_device(const osfm_match_result *r);
void osfm_result_destroy(osfm_match_result *r);

/*
 * Leaf: one pair from host buffers.  Drop-in for match_brute_force (symmetric = 0,
 * matching.py:723-756) and match_brute_force_symmetric (symmetric = 1, matching.py:759-777);
 * osfm_match_l2_ratio_ex with flags = OSFM_MATCH_SQUARED_RATIO for match_flann / match_flann_symmetric
 * (matching.py:683-720) on an exact search.
 * A: nA x dim, B: nB x dim float32 (dim must be 128; integer-valued or not, see the descriptor store).
 * out_pairs: cap x 2 int32, *out_n = number found (may exceed cap; only cap are written).
 */
int osfm_match_l2_ratio(osfm_ctx *ctx, const float *A, int nA, const float *B, int nB, int dim,
                        double ratio, int symmetric, int32_t *out_pairs, int cap, int *out_n);
int osfm_match_l2_ratio_ex(osfm_ctx *ctx, const float *A, int nA, const float *B, int nB, int dim,
                           double ratio, int symmetric, int flags, int32_t *out_pairs, int cap, int *out_n);
/* The same leaf for uint8 bit strings: match_brute_force[_symmetric] on uint8 arrays = cv2 BruteForce-Hamming (matching.py:737-740).
 * A: nA x width_bytes, B: nB x width_bytes (1..64 bytes). */
int osfm_match_hamming_ratio(osfm_ctx *ctx, const uint8_t *A, int nA, const uint8_t *B, int nB, int width_bytes,
                             double ratio, int symmetric, int32_t *out_pairs, int cap, int *out_n);
/* ... with flags: OSFM_MATCH_SQUARED_RATIO = match_flann / match_flann_symmetric on bit strings (matching.py:683-720; features.py:660-667 builds
 * cv2's LSH index for uint8 descriptors): searched exactly here, the test `d0 < lowes_ratio ** 2 * d1` in doubles on the int Hamming distances,
 * one-way matching queries with B (round 6) */
int osfm_match_hamming_ratio_ex(osfm_ctx *ctx, const uint8_t *A, int nA, const uint8_t *B, int nB, int width_bytes,
                                double ratio, int symmetric, int flags, int32_t *out_pairs, int cap, int *out_n);

/*
 * Leaf: cv2.findFundamentalMat(p1, p2, FM_RANSAC, thr, conf) as used by
 * robust_match_fundamental (matching.py:780-802).  p1, p2: n x 2 float64.
 * Returns OSFM_OK with *found = 1 (F row-major, mask n bytes) or *found = 0 (F is None).
 * n >= 15: RANSAC; 8 <= n < 15: the LMedS registrator cv2 switches to; n == 7: OSFM_E_UNSUPPORTED
 * (the reference never calls with fewer than 8 matches, matching.py:787).
 */
int osfm_ransac_fundamental(osfm_ctx *ctx, const double *p1, const double *p2, int n, double thr,
                            double conf, int max_iters, double F[9], uint8_t *mask, int *found,
                            int *iters_run_or_null);

/* ==========================================================================================
 * Bundle adjustment.  Replaces pysfm.BAHelpers.bundle (opensfm/src/sfm/src/ba_helpers.cc:581-763,
 * python seam opensfm/reconstruction.py:69-86) == bundle::BundleAdjuster::Run
 * (opensfm/src/bundle/src/bundle_adjuster.cc:595-1121) for the residual families BAHelpers::Bundle
 * adds on a plain reconstruction: reprojection errors with a shared robust loss
 * (projection_errors.h:59-208), camera-intrinsics priors (bundle_adjuster.cc:568-593) and
 * position priors on the shot origins (bundle_adjuster.cc:745-778, identity bias).
 * Flat SoA problem; all arrays are host pointers, in/out arrays are overwritten with the optimum.
 * ========================================================================================== */
#define OSFM_LOSS_TRIVIAL 0  /* "TrivialLoss"  (bundle_adjuster.cc:414-429) */
#define OSFM_LOSS_SOFTLONE 1 /* "SoftLOneLoss" -- the reference default (config.py:241) */
#define OSFM_LOSS_HUBER 2    /* "HuberLoss"    */
#define OSFM_LOSS_CAUCHY 3   /* "CauchyLoss"   */

#define OSFM_CAMERA_PERSPECTIVE 0 /* "perspective" */
#define OSFM_CAMERA_FISHEYE 1     /* "fisheye"     */
/* the other 2-D projection types: as CONSTANT cameras only (cam_fixed = 1 + cam_ext), which is how
   BundleLocal / BundleShotPoses always use cameras (ba_helpers.cc:137,415) */
#define OSFM_CAMERA_BROWN 2          /* [k1 k2 k3 p1 p2 | focal ar cx cy]                    */
#define OSFM_CAMERA_FISHEYE_OPENCV 3 /* [k1 k2 k3 k4 | focal ar cx cy]                       */
#define OSFM_CAMERA_FISHEYE62 4      /* [k1..k6 p1 p2 | focal ar cx cy]                      */
#define OSFM_CAMERA_FISHEYE624 5     /* [k1..k6 p1 p2 s0 s1 s2 s3 | focal ar cx cy]          */
#define OSFM_CAMERA_DUAL 6           /* [transition | k1 k2 | focal]                         */
#define OSFM_CAMERA_RADIAL 7         /* [k1 k2 | focal ar cx cy]                             */
#define OSFM_CAMERA_SIMPLE_RADIAL 8  /* [k1 | focal ar cx cy]                                */
#define OSFM_CAMERA_SPHERICAL 9      /* no parameters; bearings only (osfm_pixel_bearings), not a BA camera model */

typedef struct {
  int32_t n_cameras, n_shots, n_points;
  int64_t n_obs;
  double *cam_params;        /* n_cameras x 3: k1, k2, focal (geometry/src/camera.cc:9-17)   in/out */
  const double *cam_prior;   /* n_cameras x 3                                                       */
  const double *cam_sigma;   /* n_cameras x 3: prior sd of k1, k2, focal (focal: log-ratio)         */
  const uint8_t *cam_fixed;  /* n_cameras: 1 = constant (optimize_camera_parameters False)          */
  double *shot_pose;         /* n_shots x 6: rx ry rz tx ty tz (bundle/data/pose.h:17,34-43) in/out */
  const int32_t *shot_camera;    /* n_shots                                                         */
  const uint8_t *shot_fixed;     /* n_shots or NULL                                                 */
  const double *shot_gps;        /* n_shots x 3 or NULL: prior on the origin                        */
  const double *shot_gps_sigma;  /* n_shots or NULL: sd (<= 0: no prior for that shot)              */
  double *points;                /* n_points x 3                                             in/out */
  const uint8_t *point_fixed;    /* n_points or NULL                                                */
  const int32_t *obs_shot;       /* n_obs                                                           */
  const int32_t *obs_point;      /* n_obs                                                           */
  const double *obs_xy;          /* n_obs x 2 normalized image coordinates (observation.point)     */
  const double *obs_sigma;       /* n_obs: observation.scale == std_deviation (tracking.py:108)     */
  double *reproj_err;            /* n_obs x 2 or NULL: out, residual with sigma 1                   */
  /* absolute up-vector prior (BAHelpers::Bundle with align_method orientation_prior,
     ba_helpers.cc:609-621,688-692; UpVectorError, absolute_motion_errors.h:12-39; CauchyLoss(1),
     bundle_adjuster.cc:955-970): residual (R(rotation) * up - e_z) / sd per shot */
  const double *shot_up;         /* n_shots x 3 or NULL (normalised by the library)                 */
  const double *shot_up_sigma;   /* n_shots or NULL: sd (<= 0: no prior for that shot)              */
  /* projection type per camera (geometry::ProjectionType, camera_instances.h:8-20,183-190), or NULL
     = all PERSPECTIVE.  Both supported types carry the same parameters [k1, k2, focal]:
     PerspectiveCamera = <PerspectiveProjection, Disto24, UniformScale>,
     FisheyeCamera     = <FisheyeProjection,     Disto24, UniformScale>. */
  const int32_t *cam_model;      /* n_cameras or NULL: OSFM_CAMERA_*                                */
  /* native parameters [projection][distortion][affine] (camera_instances.h:127-160), 16 per camera,
     of the constant cameras whose cam_model is >= 2; NULL when there are none */
  const double *cam_ext;         /* n_cameras x 16 or NULL                                          */
                                 /* (ComputeReprojectionErrors, bundle_adjuster.cc:1196-1208)        */
} osfm_ba_problem;

typedef struct {
  int32_t loss;               /* OSFM_LOSS_*                 config["loss_function"]           */
  double loss_threshold;      /* config["loss_function_threshold"] = 1 (config.py:243)        */
  int32_t max_iterations;     /* config["bundle_max_iterations"] = 100 (config.py:283)        */
  double function_tolerance;  /* ceres default 1e-6                                           */
  double gradient_tolerance;  /* ceres default 1e-10                                          */
  double parameter_tolerance; /* ceres default 1e-8                                           */
  double initial_radius;      /* ceres initial_trust_region_radius 1e4                        */
  int32_t verbose;            /* bit 0: one progress line per LM iteration on stderr; OSFM_BA_TIME_MATVEC: ten extra Schur
                                 mat-vecs are timed with HIP events after the solve (report: ms_matvec_total, matvec_calls) */
  double pcg_tolerance;       /* relative residual of the Schur-PCG solve (default 1e-10)     */
  int32_t pcg_max_iterations; /* default 1000                                                 */
  int32_t preconditioner;     /* 0 auto: banded block Cholesky when the shot coupling is banded
                                 (half-width <= 15 shots), else block Jacobi; 1: block Jacobi  */
  double pcg_direct_tolerance; /* relative residual at which the FIRST iterate is accepted when the preconditioner is the reduced matrix
                                * itself (exact band by cyclic reduction + exact border, or constant cameras): that iterate is a direct solve
                                * -- what Ceres' SPARSE_SCHUR stops at -- plus a line search, and lands at 1e-10 .. 1e-7 (conditioning x the
                                * rounding of the explicit block inverses).  Default 1e-6: trajectories at 1e-6 and 1e-10 agree to 4e-16 in
                                * the cost over 20 iterations at configs[4] (profiles/r06_pcg_direct_tolerance.json).  <= pcg_tolerance: no such
                                * rule.  Inexact preconditioners (block Jacobi, a truncated band, a border too wide for the exact elimination)
                                * always iterate to pcg_tolerance. */
} osfm_ba_options;
#define OSFM_BA_TIME_MATVEC 2

void osfm_ba_options_default(osfm_ba_options *o);

typedef struct {
  int32_t iterations;       /* LM iterations (successful + unsuccessful), ceres' num_iterations - 1 */
  int32_t successful_steps;
  int32_t termination;      /* 0 max iterations, 1 function tol, 2 gradient tol, 3 parameter tol,
                               4 min trust region radius, -1 failure */
  double initial_cost, final_cost;
  double rmse_normalized_initial, rmse_normalized_final; /* sqrt(mean |pi(X) - obs|^2), x max(w,h) = px */
  double seconds_total, seconds_linear_solver;           /* wall_times (ba_helpers.cc:749-753)          */
  double cost_history[256];
  int64_t pcg_iterations_total;
  double ms_matvec_total;    /* HIP-event time spent in the Schur mat-vec kernels */
  int64_t matvec_calls;
  int32_t shot_bandwidth;           /* max |shot_a - shot_b| over shots sharing a point          */
  int32_t preconditioner_bandwidth; /* block half-width of the banded preconditioner, 0 = Jacobi */
  /* wall_times of BAHelpers::Bundle (ba_helpers.cc:749-753): setup = index build + H2D,
     run = the LM loop (what ceres::Solve covers), teardown = D2H of parameters and errors */
  double seconds_setup, seconds_run, seconds_teardown;
  /* 1: the shots were renumbered internally (reverse Cuthill-McKee on the co-visibility graph) because
     the caller's order had a half-width above what the banded preconditioner holds; shot_bandwidth is
     then the half-width after renumbering and shot_bandwidth_input the caller's. */
  int32_t shots_reordered, shot_bandwidth_input;
} osfm_ba_report;

int osfm_ba_solve(osfm_ctx *ctx, osfm_ba_problem *problem, const osfm_ba_options *options,
                  osfm_ba_report *report);

/* Host-only (no GPU): the shot renumbering osfm_ba_solve applies to unordered collections (reverse
   Cuthill-McKee on the co-visibility graph) and the co-visibility half-width before / after it. */
int osfm_ba_shot_order(const osfm_ba_problem *problem, int32_t *new_of_old, int32_t *half_width_before,
                       int32_t *half_width_after);

/* ------------------------------------------------------------------------------------------
 * The general bundle adjustment: everything BAHelpers::Bundle (ba_helpers.cc:581-763) hands to bundle::BundleAdjuster and Run
 * (bundle_adjuster.cc:595-1121) solves -- every projection type with all of its native parameters free or constant
 * (camera_instances.h, AddCameraPriorError bundle_adjuster.cc:568-593 with logarithmic focal / aspect ratio, the dual camera's
 * ParameterBarrier), the SPHERICAL 3-D bearing residual (projection_errors.h:208-376), rig cameras with pose priors and rig
 * instances (error_utils.h:68-85 WorldToCameraCoordinatesRig), rig instance position priors through a per-camera GPS bias
 * (SimilarityPriorTransform, bias.h:33-53, bundle_adjuster.cc:745-778), point priors = ground control points
 * (bundle_adjuster.cc:688-707, ba_helpers.cc:349-406), absolute up vectors (absolute_motion_errors.h:12-39, Cauchy(1)), compass /
 * inclinometer priors, depth priors.
 * Round 5: this entry point runs on the SAME streaming Schur solver as osfm_ba_solve (its generic mode, csrc/ba_generic.inc): points
 * eliminated on the fly, the rig instances in a co-visibility band factorised exactly (cyclic reduction), the free rig cameras /
 * camera intrinsics / biases as a border of up to 64 unknowns eliminated exactly (wider borders: preconditioned CG) -- time and
 * memory linear in the observations, BASELINE configs[4] size with a BROWN camera in one call.  (Round 4 formed the reduced system
 * densely and factorised it with rocSOLVER: n_r^2 doubles.)  osfm_ba_solve above remains the specialisation for the perspective /
 * fisheye [k1 k2 focal] configuration the headline BA figure is quoted on.
 * Poses are CAM_TO_WORLD [rx ry rz tx ty tz] (bundle/data/pose.h:17,34-43); camera parameters in the native order of the
 * OSFM_CAMERA_* definitions, 16 slots per camera; in/out arrays are overwritten with the optimum.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int32_t n_cameras;
  const int32_t *cam_model;        /* n_cameras: OSFM_CAMERA_*                                                         */
  double *cam_params;              /* n_cameras x 16                                                            in/out */
  const double *cam_prior;         /* n_cameras x 16                                                                   */
  const double *cam_sigma;         /* n_cameras x 16: GetDefaultCameraSigma (bundle_adjuster.cc:47-69)                 */
  const uint8_t *cam_fixed;        /* n_cameras                                                                        */
  double *bias;                    /* n_cameras x 7 [rx ry rz tx ty tz scale] (bias.h:10-31) or NULL = identity  in/out */
  const uint8_t *bias_fixed;       /* n_cameras or NULL = all constant (AddCamera's default, bundle_adjuster.cc:98-106) */
  int32_t n_rig_cameras;
  double *rig_camera_pose;         /* n_rig_cameras x 6                                                          in/out */
  const double *rig_camera_prior;  /* n_rig_cameras x 6 or NULL                                                         */
  const double *rig_camera_sigma;  /* n_rig_cameras x 6 or NULL (GetDefaultRigPoseSigma)                                */
  const uint8_t *rig_camera_fixed; /* n_rig_cameras                                                                     */
  int32_t n_rig_instances;
  double *rig_instance_pose;       /* n_rig_instances x 6                                                        in/out */
  const uint8_t *rig_instance_fixed;       /* n_rig_instances or NULL                                                   */
  const double *rig_instance_gps;          /* n_rig_instances x 3 or NULL: AddRigInstancePositionPrior                  */
  const double *rig_instance_gps_sigma;    /* n_rig_instances x 3; [3 i] <= 0: no prior for instance i                  */
  const int32_t *rig_instance_bias_camera; /* n_rig_instances: the camera whose bias applies (its first shot's camera,
                                              bundle_adjuster.cc:757-764)                                               */
  int32_t n_shots;
  const int32_t *shot_rig_instance, *shot_rig_camera, *shot_camera; /* n_shots each                                     */
  const double *shot_up;           /* n_shots x 3 or NULL: AddAbsoluteUpVector                                          */
  const double *shot_up_sigma;     /* n_shots; <= 0: none                                                               */
  int32_t n_points;
  double *points;                  /* n_points x 3                                                               in/out */
  const uint8_t *point_fixed;      /* n_points or NULL                                                                  */
  const double *point_prior;       /* n_points x 3 or NULL: AddPointPrior                                               */
  const double *point_prior_sigma; /* n_points x 3; [3 p] <= 0: no prior for point p                                    */
  const uint8_t *point_prior_has_altitude; /* n_points or NULL = all 1: 0 constrains x, y only                          */
  int64_t n_obs;
  const int32_t *obs_shot, *obs_point;
  const double *obs_xy;            /* n_obs x 2 normalized image coordinates                                            */
  const double *obs_sigma;         /* n_obs                                                                             */
  double *reproj_err;              /* n_obs x 3 or NULL: out, residual with sigma 1 (third component: spherical only)   */
  /* compass / inclinometer priors per shot (AddAbsolutePan / Tilt / Roll, absolute_motion_errors.h:40-137, Cauchy(1)):
     angle in radians and its sd (<= 0: none); NULL = none at all */
  const double *shot_pan, *shot_pan_sigma, *shot_tilt, *shot_tilt_sigma, *shot_roll, *shot_roll_sigma;
  /* depth priors of the observations (map::Depth, observation.h:10-18; AddPointProjectionObservation's depth_prior argument as
     BAHelpers passes it, ba_helpers.cc:695-696): RelativeDepthError (bundle/error/relative_depth_error.h, bundle_adjuster.cc:497-528),
     one residual (depth_in_camera - depth) / sd per observation that has one, depth_in_camera = |X_cam| (radial) or its z, under the
     point-projection loss.  n_obs each; obs_depth_sigma[o] <= 0: none; obs_depth / obs_depth_sigma NULL: none at all;
     obs_depth_radial NULL: all radial.  A non-finite depth with a positive sd is OSFM_E_INVALID (the reference throws). */
  const double *obs_depth, *obs_depth_sigma;
  const uint8_t *obs_depth_radial;
} osfm_bundle_problem;

int osfm_bundle_solve(osfm_ctx *ctx, osfm_bundle_problem *problem, const osfm_ba_options *options, osfm_ba_report *report);

/* =====================================================================================
 * Tracks (next row after the hot path: SURVEY.md 8f-1)
 * Replaces the grouping of tracking.create_tracks_manager (opensfm/tracking.py:68-98, union-find
 * opensfm/unionfind.py:67-103, _good_track tracking.py:238-244): links every match
 * (im1, f1) -- (im2, f2) into connected components, lists the components in the order of their
 * first-inserted member, members in insertion order, keeps those with >= min_length members and
 * no image twice; track_id = index in that list.
 * edge_a/edge_b: global node ids in the reference's union order (pair by pair, match by match);
 * node id of feature f of image i = node_offsets[i] + f; node_offsets has n_images + 1 entries.
 * ===================================================================================== */
typedef struct osfm_tracks osfm_tracks;
int osfm_tracks_create(osfm_ctx *ctx, const int32_t *edge_a, const int32_t *edge_b, int64_t n_edges,
                       const int64_t *node_offsets, int32_t n_images, int32_t min_length, osfm_tracks **out);
int64_t osfm_tracks_num_tracks(const osfm_tracks *t);
int64_t osfm_tracks_num_observations(const osfm_tracks *t);
double osfm_tracks_device_ms(const osfm_tracks *t); /* HIP-event time of the device part */
/* each n_observations long, grouped by track in track order, members in insertion order */
int osfm_tracks_fetch(const osfm_tracks *t, int32_t *obs_track, int32_t *obs_image, int32_t *obs_feature);
void osfm_tracks_destroy(osfm_tracks *t);

/* =====================================================================================
 * Calibrated robust matching (row M-a9 / SURVEY.md 8f-3): essential-matrix LO-RANSAC on bearings.
 * Organisation (round 2, relpose.hip / relpose_rounds.h): all pairs of a call go through rounds of kernels together -- walk (one
 * wavefront per pair: scoring, the reference's decision rules, the draws), solve5a / solve5b / solveN (one lane per minimal /
 * non-minimal problem), pose (one lane per essential matrix) -- then one launch of the refinement stage.  The numerics and the
 * round logic are pinned bit for bit against the CPU oracle by a host emulation (tests/test_relpose_core_host.py); on the MI355X
 * the RANSAC stage is bit-identical to the oracle and the inlier sets after the refinement are identical
 * (tests/test_gpu_zz_relpose.py).  128 k pairs / s at 300 correspondences per pair in 16 k-pair calls, 180 k in 64 k-pair calls
 * (profiles/r02_relpose_*.json).
 *
 * osfm_pixel_bearings  replaces camera.pixel_bearing_many(points) (opensfm/src/geometry/camera.cc ->
 *   ProjectGeneric::Backward, camera_instances.h:154-160) for every OSFM_CAMERA_* model; cam = the model's
 *   parameters in the native order listed at the OSFM_CAMERA_* definitions ([k1, k2, focal] for PERSPECTIVE /
 *   FISHEYE, may be NULL for SPHERICAL); px: n x 2 normalised image coordinates, bearings: n x 3.
 *   (MI355X vs oracle, profiles/r01_guided_bringup.txt: bit-identical for the perspective-projection models, <= 2.3e-16
 *   for those that go through the device sin / cos / tan.)
 * osfm_relpose_pairs   a batch of pairs; pair p owns the correspondences offsets[p] .. offsets[p+1]-1 of the
 *   concatenated bearing arrays b1, b2 (total x 3, doubles, second-image bearing y and first-image bearing x
 *   with y ~ R x + t for the models below).
 *   mode OSFM_RELPOSE_RANSAC: pyrobust.ransac_relative_pose(b1, b2, threshold, params, RANSAC)
 *     (opensfm/src/robust/src/instanciations.cc:33-48, robust_estimator.h:37-119): result.model / lo_model
 *     (3 x 4 row-major), score, iterations; mask = inliers of the best score.
 *   mode OSFM_RELPOSE_MATCH: the body of matching.robust_match_calibrated after the bearings
 *     (opensfm/matching.py:886-903): RANSAC, three rounds of compute_inliers_bearings (4, 2, 1 x threshold)
 *     + relative_pose_refinement, final compute_inliers_bearings; mask = the inliers the reference keeps
 *     (all zero where it returns an empty array), R / t = pose of the second camera in the first.
 *   The sampler is std::mt19937(42) with std::uniform_int_distribution as libstdc++ >= 11 implements it (Lemire's
 *   multiply-shift); ties between scores keep the newcomer (std::max).  Both are pinned against the reference's own
 *   robust_estimator.h / random_sampler.h compiled on the build box (oracle/_ref).
 * ===================================================================================== */
enum { OSFM_RELPOSE_RANSAC = 0, OSFM_RELPOSE_MATCH = 1 };
typedef struct osfm_relpose_params {
  double threshold;          /* radians: config robust_matching_calib_threshold (0.004) */
  double probability;        /* RobustEstimatorParams::probability (0.99; the Python caller never sets it) */
  int32_t iterations;        /* 1000 (matching.py:889) */
  int32_t use_lo;            /* RobustEstimatorParams::use_local_optimization (1) */
  int32_t lo_iterations;     /* ::local_optimization_iterations (10) */
  int32_t refine_iterations; /* config five_point_refine_match_iterations (10) */
} osfm_relpose_params;
typedef struct osfm_relpose_result {
  double model[12], lo_model[12]; /* ScoreInfo::model / lo_model, [R | t] row-major */
  double R[9], t[3];              /* MATCH mode: after the last refinement (zeros when rejected) */
  int32_t score, iterations;      /* best inlier count of the RANSAC, iterations it ran */
  int32_t n_inliers, pad;         /* number of ones in this pair's mask */
} osfm_relpose_result;
int osfm_pixel_bearings(osfm_ctx *ctx, int model, const double *cam, const double *px, int n, double *bearings);
int osfm_relpose_pairs(osfm_ctx *ctx, const double *b1, const double *b2, const int64_t *offsets, int n_pairs,
                       const osfm_relpose_params *params, int mode, osfm_relpose_result *results, uint8_t *mask,
                       double *kernel_ms /* may be NULL: HIP-event time of the kernels */);

/* =====================================================================================
 * Rotation-only LO-RANSAC of image pairs (reconstruction.compute_image_pairs): the ranking of candidate initial
 * pairs of `opensfm reconstruct`.  relrot.hip / relrot_core.h (the walk of Estimate too; its sampler: loransac_walk.h): one wavefront per pair (lane
 * 0 draws the next block of samples, one 3-point model per lane, the wavefront scores each model over the pair's correspondences
 * in the reference's order); the same launch computes the rotation-only inlier count and the reconstructability score.  The per-pair
 * walk is pinned bit for bit by a host build of the same headers (tests/test_relrot_host.py) against a sequential restatement on std::mt19937 and
 * against the reference's robust_estimator.h; the GPU is pinned against that host build (tests/test_gpu_relrot.py).
 *
 * osfm_relrot_pairs   pyrobust.ransac_relative_rotation(b1, b2, threshold, params, RANSAC) for every pair of a batch
 *   (robust/src/instanciations.cc:50-64 -> Estimate<RansacScoring, RelativeRotation>, robust_estimator.h:37-119): pair p owns
 *   the correspondences offsets[p] .. offsets[p+1]-1 of b1 / b2 (total x 3, first / second of the samples, used as given).
 *   Sampler std::mt19937(42) with libstdc++'s uniform_int_distribution, ties keep the newcomer, LO on every new or tied best
 *   with >= 3 inliers (sample size max(min(12, inliers / 2), 3)), ShouldStop with exponent 3 -- as osfm_relpose_pairs.
 *   result.model / lo_model: ScoreInfo::model / lo_model (3 x 3 row-major; multiview.relative_pose_ransac_rotation_only returns
 *   lo_model^T); score; iterations run.  mask (total bytes, may be NULL): the inliers of the best score.
 *   params.inlier_chord > 0: also _two_view_rotation_inliers(b1, b2, lo_model^T, chord) (reconstruction.py:377-384,
 *   |lo_model^T b2 - b1| < chord) -> n_rotation_inliers, and pairwise_reconstructability(n, n_rotation_inliers)
 *   (reconstruction.py:193-200) -> reconstructability; inlier_chord <= 0: n_rotation_inliers = -1, reconstructability = 0.
 *   n_pairs == 0 returns OSFM_OK and touches nothing.  A pair with fewer than 3 correspondences (zero-length included) is
 *   OSFM_E_INVALID: the reference's sampler never returns there (it cannot draw 3 distinct indices).
 * osfm_relrot_pairs_pixels   the same from normalised image coordinates p1 / p2 (total x 2): the bearings are computed on the
 *   device (camera.pixel_bearing_many, as osfm_pixel_bearings) with the cameras pair_cams[2p], pair_cams[2p+1] of the table
 *   cam_model[n_cams] (OSFM_CAMERA_*) / cam_params[n_cams x 16] (native parameter order, as osfm_match_pairs_calibrated).
 *   kernel_ms then includes the bearings.
 * ===================================================================================== */
typedef struct osfm_relrot_params {
  double threshold;                /* radians: 4 * config five_point_algo_threshold in compute_image_pairs (0.016) */
  double probability;              /* RobustEstimatorParams::probability (0.99: relative_pose_ransac_rotation_only never sets it) */
  double inlier_chord;             /* chord of the rotation-only inlier count (compute_image_pairs: the threshold); <= 0: skipped */
  int32_t iterations;              /* 1000 (reconstruction.py:409) */
  int32_t use_lo;                  /* RobustEstimatorParams::use_local_optimization (1) */
  int32_t lo_iterations;           /* ::local_optimization_iterations (10) */
  int32_t use_iteration_reduction; /* ::use_iteration_reduction (1) */
} osfm_relrot_params;
typedef struct osfm_relrot_result {
  double model[9], lo_model[9];        /* ScoreInfo::model / lo_model, row-major */
  int32_t score, iterations;           /* best inlier count, iterations run */
  int32_t n_rotation_inliers;          /* |lo_model^T b2 - b1| < inlier_chord; -1 when skipped */
  int32_t reconstructability;          /* pairwise_reconstructability(n, n_rotation_inliers); 0 when skipped */
} osfm_relrot_result;
int osfm_relrot_pairs(osfm_ctx *ctx, const double *b1, const double *b2, const int64_t *offsets, int n_pairs, const osfm_relrot_params *params,
                      osfm_relrot_result *results, uint8_t *mask_or_null, double *kernel_ms /* may be NULL: HIP-event time */);
int osfm_relrot_pairs_pixels(osfm_ctx *ctx, const double *p1, const double *p2, const int64_t *offsets, int n_pairs, const int32_t *pair_cams,
                             const int32_t *cam_model, const double *cam_params, int n_cams, const osfm_relrot_params *params,
                             osfm_relrot_result *results, uint8_t *mask_or_null, double *kernel_ms /* may be NULL */);

/* =====================================================================================
 * Two-view 5-point reconstruction of candidate initial pairs (reconstruction.bootstrap_reconstruction ->
 * two_view_reconstruction_general, opensfm/reconstruction.py:488-534, without its plane-based branch): a batch of ranked pairs in one
 * call.  twoview.hip / twoview_core.h; no solver of its own -- the LO-RANSAC is osfm_relpose_pairs' (mode OSFM_RELPOSE_RANSAC, its
 * results stay on the device), the inlier test, the rand() picks, the TinySolver refinement and the angle-axis are the leaves of
 * relpose_core.h that the calibrated matcher is pinned on.  tv_config_kernel: one wavefront per (pair, configuration);
 * tv_decide_kernel: one thread per pair.  A host build of twoview_core.h is held bit for bit to a restatement composed from the CPU
 * oracle's leaves (tests/test_twoview_host.py); the GPU to that host build: statuses, choices, masks and the RANSAC bit for bit, the
 * refined poses to 1e-6 (tests/test_gpu_twoview.py).
 *
 * osfm_two_view_pairs   pair p owns the correspondences offsets[p] .. offsets[p+1]-1 of the bearings b1 / b2 (total x 3).
 *   poses == NULL: multiview.relative_pose_ransac(b1, b2, threshold, ransac_iterations, .) (multiview.py:494-516: R = R_lo^T,
 *     t = -R_lo^T t_lo of the RANSAC's lo_model), then two_view_reconstruction_5pt on that pose.
 *   poses given (n_pairs x 12: R row-major, then t): two_view_reconstruction_5pt(b1, b2, R, t, threshold, refine_iterations,
 *     check_reversal, reversal_ratio) (reconstruction.py:415-485); no RANSAC runs.
 *   Per configuration (0: the pose as given; 1, only with check_reversal: R^T, -R^T t) two_view_reconstruction_and_refinement
 *   (reconstruction.py:336-374): compute_inliers_bearings, with more than 5 inliers relative_pose_optimize_nonlinear on them
 *   (srand(42) restarts per refinement, as in the reference) and the inliers again.  result.R[c] / t[c]: R_curr^T (what the
 *   reference hands to cv2.Rodrigues) and -R_curr^T t_curr.  Then the choice (reconstruction.py:458-485): a configuration counts
 *   with more than 5 inliers; of two, min / max > reversal_ratio is undecidable, else the one with more inliers, a tie picking
 *   configuration 1.  rotation: ceres' RotationMatrixToAngleAxis of the chosen R (cv2.Rodrigues' bit patterns are not pinned).
 *   mask (total bytes): bit 0 / 1 = inlier of configuration 0 / 1, bit 2 = inlier of the chosen configuration.
 *   A pair of 5 or fewer correspondences can never count: OSFM_TWO_VIEW_NO_CONFIGURATION, n_inliers -1, no work (it reaches
 *   neither the RANSAC nor the device).  n_pairs == 0 returns OSFM_OK and touches nothing.  Arguments are checked as by
 *   osfm_relpose_pairs (OSFM_E_INVALID: n_pairs < 0, offsets that do not start at 0 or descend, null bearings).
 * osfm_two_view_pairs_pixels   the same from normalised image coordinates p1 / p2 (total x 2) and the camera table of
 *   osfm_relrot_pairs_pixels (pair_cams[2p], pair_cams[2p+1]; cam_model[n_cams]; cam_params[n_cams x 16]); kernel_ms then includes
 *   the bearings.
 * ===================================================================================== */
enum { OSFM_TWO_VIEW_OK = 0, OSFM_TWO_VIEW_NO_CONFIGURATION = 1, OSFM_TWO_VIEW_UNDECIDABLE = 2 };
typedef struct osfm_two_view_params {
  double threshold;          /* radians: config five_point_algo_threshold (0.004) */
  double probability;        /* RobustEstimatorParams::probability (0.99: relative_pose_ransac never passes its 0.999 on) */
  double reversal_ratio;     /* config five_point_reversal_ratio (0.95) */
  int32_t ransac_iterations; /* 1000 (reconstruction.py:522) */
  int32_t use_lo;            /* RobustEstimatorParams::use_local_optimization (1) */
  int32_t lo_iterations;     /* ::local_optimization_iterations (10) */
  int32_t refine_iterations; /* config five_point_refine_rec_iterations (1000) */
  int32_t check_reversal;    /* config five_point_reversal_check */
  int32_t skip_inlier_tests; /* 0.  1: every correspondence counts as an inlier before and after the refinement -- configuration 0
                                on a given pose is then pygeometry.relative_pose_refinement on its own */
} osfm_two_view_params;
typedef struct osfm_two_view_result {
  double R[2][9], t[2][3];            /* per configuration (zeros for one that was not run) */
  double rotation[3], translation[3]; /* the chosen configuration: angle-axis of its R, its t; zeros unless status is OK */
  double lo_model[12];                /* the RANSAC's ScoreInfo::lo_model (zeros on given poses) */
  int32_t status, chosen;             /* OSFM_TWO_VIEW_*; -1, 0 or 1 */
  int32_t n_inliers[2];               /* per configuration; -1 when not run */
  int32_t refine_iterations[2];       /* TinySolver iterations per configuration (0: not refined) */
  int32_t score, iterations;          /* best inlier count of the RANSAC, iterations it ran (zeros on given poses) */
} osfm_two_view_result;
int osfm_two_view_pairs(osfm_ctx *ctx, const double *b1, const double *b2, const int64_t *offsets, int n_pairs, const double *poses_or_null,
                        const osfm_two_view_params *params, osfm_two_view_result *results, uint8_t *mask,
                        double *kernel_ms /* may be NULL: HIP-event time of the kernels */);
int osfm_two_view_pairs_pixels(osfm_ctx *ctx, const double *p1, const double *p2, const int64_t *offsets, int n_pairs, const int32_t *pair_cams,
                               const int32_t *cam_model, const double *cam_params, int n_cams, const double *poses_or_null,
                               const osfm_two_view_params *params, osfm_two_view_result *results, uint8_t *mask, double *kernel_ms /* may be NULL */);

/* =====================================================================================
 * Plane-based two-view reconstruction of candidate initial pairs: the other half of two_view_reconstruction_general
 * (reconstruction.two_view_reconstruction_plane_based, opensfm/reconstruction.py:298-333), a batch of ranked pairs in one call.
 * plane.hip / plane_core.h.  pl_ransac_kernel: one wavefront per pair -- x = (b0 / b2, b1 / b2) per side (multiview.euclidean), a
 * homography by this project's LO-RANSAC walk (loransac_walk.h; std::mt19937(42), 4-point samples, one model per sample, LO on every
 * new or tied best with >= 4 inliers, ShouldStop with exponent 4) over a normalised DLT with cv2.findHomography's inlier test (one-way
 * transfer error in the second image below the threshold), a final fit over all inliers kept when it has at least as many, H scaled
 * to middle singular value 1 and positive determinant, multiview.motion_from_plane_homography restated (multiview.py:366-441) with the
 * signs of the singular vectors fixed.  pl_motion_kernel: one wavefront per (pair, motion), compute_inliers_bearings with R^T, -R^T t.
 * pl_decide_kernel: one thread per pair.  NOT cv2's RANSAC, refit with LM or float32 points (plane_core.h says what is and is not
 * restated), and the motion returned is the one with the most inliers, the lowest index on ties -- the reference's np.argmax over a
 * map object always returns motion 0.  A host build of plane_core.h is held to a numpy restatement (tests/test_plane_host.py), the
 * GPU to that host build bit for bit (tests/test_gpu_plane.py).
 *
 * osfm_two_view_plane_pairs   pair p owns the correspondences offsets[p] .. offsets[p+1]-1 of the bearings b1 / b2 (total x 3).  A row
 *   with b2 <= 0 on either side keeps its place and is an inlier of no homography.  status: OSFM_PLANE_OK; NO_HOMOGRAPHY: no model
 *   with at least 4 inliers (H, singular zero, h_inliers 0); DEGENERATE: the reference's "two singular values within 1.0001" (pure
 *   rotation, a plane through a camera centre) or H of rank below 2 (H, singular and h_inliers are reported).  Unless OK: chosen -1,
 *   motion_inliers, R, t, rotation, translation zero.  R, t: the picked motion (x2 ~ R x1 + t, t in units of the plane's distance);
 *   rotation: ceres' RotationMatrixToAngleAxis of R (the reference applies cv2.Rodrigues to R, not to R^T).
 *   mask (total bytes): bit 0 = inlier of H, bit 1 = inlier of the picked motion.
 *   A pair of fewer than 4 correspondences never reaches the device: NO_HOMOGRAPHY, chosen -1, mask 0.  n_pairs == 0 returns OSFM_OK
 *   and touches nothing.  OSFM_E_INVALID (null arguments, offsets that do not start at 0 or descend, threshold <= 0, a camera outside
 *   the table): no output is touched, kernel_ms included.
 * osfm_two_view_plane_pairs_pixels   the same from normalised image coordinates p1 / p2 (total x 2) and the camera table of
 *   osfm_two_view_pairs_pixels; kernel_ms then includes the bearings.
 * osfm_homography_solve   the leaf: the normalised DLT over all n >= 4 rows of x1 / x2 (n x 2), *ok_out 0 (H_out zero) or 1.
 * osfm_plane_motions   the leaf: the decomposition of H (row-major); motions_out: 8 x (R (9), t (3), n (3), d), *count_out 0 or 8.
 * ===================================================================================== */
enum { OSFM_PLANE_OK = 0, OSFM_PLANE_NO_HOMOGRAPHY = 1, OSFM_PLANE_DEGENERATE = 2 };
typedef struct osfm_plane_params {
  double threshold;                /* of the transfer error (normalised coordinates) and of the bearings' test (radians): 0.004 */
  double probability;              /* RobustEstimatorParams::probability (0.99) */
  int32_t iterations;              /* ::iterations (1000) */
  int32_t use_lo;                  /* ::use_local_optimization (1) */
  int32_t lo_iterations;           /* ::local_optimization_iterations (10) */
  int32_t use_iteration_reduction; /* ::use_iteration_reduction (1) */
} osfm_plane_params;
typedef struct osfm_plane_result {
  double H[9], singular[3];                        /* the homography (row-major) and its singular values (middle one 1) */
  double R[9], t[3], rotation[3], translation[3];  /* the picked motion; rotation: angle-axis of R, translation: t */
  int32_t status, chosen;                          /* OSFM_PLANE_*; -1 or 0 .. 7 */
  int32_t h_inliers, iterations, n_inliers;        /* inliers of H, iterations of the walk, inliers of the picked motion */
  int32_t motion_inliers[8];                       /* per motion, in the reference's loop order */
  int32_t pad;
} osfm_plane_result;
int osfm_two_view_plane_pairs(osfm_ctx *ctx, const double *b1, const double *b2, const int64_t *offsets, int n_pairs,
                              const osfm_plane_params *params, osfm_plane_result *results, uint8_t *mask,
                              double *kernel_ms /* may be NULL: HIP-event time of the kernels */);
int osfm_two_view_plane_pairs_pixels(osfm_ctx *ctx, const double *p1, const double *p2, const int64_t *offsets, int n_pairs,
                                     const int32_t *pair_cams, const int32_t *cam_model, const double *cam_params, int n_cams,
                                     const osfm_plane_params *params, osfm_plane_result *results, uint8_t *mask, double *kernel_ms /* may be NULL */);
int osfm_homography_solve(osfm_ctx *ctx, const double *x1, const double *x2, int n, double *H_out, int *ok_out);
int osfm_plane_motions(osfm_ctx *ctx, const double *H, double *motions_out /* 8 x 16 doubles */, int *count_out);

/* =====================================================================================
 * Absolute-pose (P3P) LO-RANSAC of candidate images (reconstruction.resect, opensfm/reconstruction.py:695-762): the step of
 * grow_reconstruction that adds an image to the map.  abspose.hip / abspose_core.h, the same walk (loransac_walk.h): one wavefront per image (lane 0 draws the next
 * block of samples, four lanes per sample solve one root of the three-point solver's quartic each, the wavefront scores every model
 * over the image's rows in the reference's order; the Lu-Hager solves of a local optimisation run one per lane); the same launch
 * applies resect's inlier test.  The decision path uses + - * / sqrt only (the quartic's complex square and cube roots included), so
 * the walk is pinned bit for bit by a host build of the same headers (tests/test_abspose_host.py) against a sequential restatement
 * on std::mt19937 and against the reference's robust_estimator.h; the GPU is pinned against that host build
 * (tests/test_gpu_abspose.py).  What is not pinned: Eigen's and libstdc++'s last bits (abspose_core.h says which).
 *
 * osfm_abspose_images   pyrobust.ransac_absolute_pose(bearings, points, threshold, params, RANSAC) for every image of a batch
 *   (robust/src/instanciations.cc:67-83 -> Estimate<RansacScoring, AbsolutePose>): image i owns the rows offsets[i] .. offsets[i+1]-1
 *   of bearings / points (total x 3).  Sampler std::mt19937(42), 0 or 4 models per sample scored in order, ties keep the newcomer, LO
 *   on every new or tied best with >= 3 inliers, ShouldStop with exponent 3 after every model.
 *   result.model / lo_model: ScoreInfo::model / lo_model ([R | t], 3 x 4 row-major; all zero when no sample gave a model); score;
 *   iterations run.  ransac_mask (total bytes, may be NULL): the inliers of the best score.
 *   params.inlier_chord > 0: resect's test on T = [R^T | -R^T t] of lo_model (multiview.absolute_pose_ransac):
 *   |normalized(R (X - o)) - b| < chord -> num_inliers and chord_mask (total bytes, may be NULL); <= 0: num_inliers = -1, mask zero.
 *   n_images == 0 returns OSFM_OK and touches nothing.  An image with fewer than 3 rows is OSFM_E_INVALID: the reference's sampler
 *   never returns there (resect itself returns before the call below 5 rows).
 * osfm_abspose_images_pixels   the same from normalised image coordinates xy (total x 2): the bearings are computed on the device
 *   with camera image_cam[i] of the table cam_model[n_cams] (OSFM_CAMERA_*) / cam_params[n_cams x 16].  kernel_ms includes them.
 * osfm_abspose_solve   the leaf solvers: kind 0 = geometry.absolute_pose_three_points on rows 0 .. 2 (models_out: 4 x 12, *count_out
 *   0 or 4; models [R^T | -R^T t] as the reference returns them), kind 1 = geometry.absolute_pose_n_points on all n rows
 *   (models_out: 12, *count_out = 1).
 * ===================================================================================== */
typedef struct osfm_abspose_params {
  double threshold;                /* radians: config resection_threshold in resect (0.004) */
  double probability;              /* RobustEstimatorParams::probability (0.99: absolute_pose_ransac never sets it) */
  double inlier_chord;             /* chord of resect's inlier test (resect: the threshold); <= 0: skipped */
  int32_t iterations;              /* 1000 (reconstruction.py:725) */
  int32_t use_lo;                  /* RobustEstimatorParams::use_local_optimization (1) */
  int32_t lo_iterations;           /* ::local_optimization_iterations (10) */
  int32_t use_iteration_reduction; /* ::use_iteration_reduction (1) */
} osfm_abspose_params;
typedef struct osfm_abspose_result {
  double model[12], lo_model[12];      /* ScoreInfo::model / lo_model, 3 x 4 row-major */
  int32_t score, iterations;           /* best inlier count, iterations run */
  int32_t num_inliers;                 /* resect's inliers; -1 when skipped */
} osfm_abspose_result;
int osfm_abspose_images(osfm_ctx *ctx, const double *bearings, const double *points, const int64_t *offsets, int n_images,
                        const osfm_abspose_params *params, osfm_abspose_result *results, uint8_t *ransac_mask_or_null,
                        uint8_t *chord_mask_or_null, double *kernel_ms /* may be NULL: HIP-event time */);
int osfm_abspose_images_pixels(osfm_ctx *ctx, const double *xy, const double *points, const int64_t *offsets, int n_images,
                               const int32_t *image_cam, const int32_t *cam_model, const double *cam_params, int n_cams,
                               const osfm_abspose_params *params, osfm_abspose_result *results, uint8_t *ransac_mask_or_null,
                               uint8_t *chord_mask_or_null, double *kernel_ms /* may be NULL */);
int osfm_abspose_solve(osfm_ctx *ctx, const double *bearings, const double *points, int n, int kind, double *models_out, int *count_out);

/*
 * Batched pair matching for the pairs that take the calibrated branch of robust_match (opensfm/matching.py:906-929: every pair with
 * a camera that is not an undistorted perspective / brown one): per pair matching.match (matching.py:563-634) = descriptor stage,
 * the robust_matching_min_match gate, robust_match_calibrated (matching.py:871-903) on the bearings of the matched features, the
 * gate again.  cam_model[n_images] (OSFM_CAMERA_*) and cam_params[n_images x 16] (native parameter order, as osfm_pixel_bearings)
 * describe the camera of every image of the store.  Everything between the two stages stays on the device: bearings of all features
 * once per call, gather of the matched bearings, the LO-RANSAC / refinement rounds, ordered compaction of the inliers.
 * Same result object as osfm_match_pairs.
 */
int osfm_match_pairs_calibrated(osfm_ctx *ctx, const osfm_store *store, const int32_t *cam_model, const double *cam_params,
                                const int32_t *pairs, int64_t n_pairs, const osfm_match_params *params,
                                const osfm_relpose_params *relpose, osfm_match_result **out, osfm_match_timings *timings_or_null);

/* =====================================================================================
 * Masked / guided descriptor matching (second half of row M-a9 / SURVEY.md 8f-3).
 * Drop-in for match_brute_force(f1, f2, config, maskij) (symmetric = 0, opensfm/matching.py:723-756) and
 * match_brute_force_symmetric(fi, fj, config, maskij) (symmetric = 1, matching.py:759-777: the reverse direction uses
 * the transposed mask).  The mask is EITHER explicit (mask: n1 x n2 bytes, non-zero = allowed) OR, with mask == NULL,
 * the epipolar mask of guided matching evaluated on the fly (never materialised):
 *   compute_inliers_bearing_epipolar(b1, b2, pose, threshold) (matching.py:847-868 ->
 *   geometry::EpipolarAngleTwoBearingsMany, opensfm/src/geometry/src/triangulation.cc:195-219) with b1 / b2 the float32
 *   bearings of the two images, R = pose.get_R_cam_to_world() (row-major), t = pose.get_origin() of the relative pose
 *   (pose2.relative_to(pose1), matching.py:204-207), threshold = config guided_matching_threshold (radians).
 * f1: n1 x dim, f2: n2 x dim float32 (integer-valued in [0, 255], dim must be 128); out_pairs: cap x 2 int32 sorted by
 * (i, j); *out_n = number found (may exceed cap; only cap are written).
 * This single-pair leaf takes integer-valued descriptors only (it is what the Python leaves match_brute_force[_symmetric](maskij)
 * call); float descriptors go through the batched entry point below, whose store keeps their float rows.
 * ===================================================================================== */
int osfm_match_guided(osfm_ctx *ctx, const float *f1, int n1, const float *f2, int n2, int dim, const uint8_t *mask,
                      const float *b1, const float *b2, const double *R, const double *t, double threshold, double ratio,
                      int symmetric, int32_t *out_pairs, int cap, int *out_n);

/*
 * Guided matching for a whole pair list over the resident store: the body of match_images_with_pairs when `poses` are given
 * (opensfm/matching.py:63-98 -> match_unwrap_args :204-207 -> match() :563-634 with _match_descriptors_guided_impl :260-337):
 * per pair the epipolar mask compute_inliers_bearing_epipolar (:847-868), match_brute_force[_symmetric] under that mask, the
 * robust_matching_min_match gates and robust_match -- descriptor stage in three launches per chunk of pairs (guided.hip), robust
 * stage as in osfm_match_pairs (params->robust: fundamental-matrix RANSAC) or osfm_match_pairs_calibrated (cam_model / cam_params /
 * relpose given; otherwise pass all three as NULL).
 * bearings: sum(counts) x 3 float32 in the store's image / feature order (feature_loader.load_bearings);
 * poses:    n_pairs x 12, per pair R = relative_pose.get_R_cam_to_world() (row-major) then t = relative_pose.get_origin(),
 *           relative_pose = pose2.relative_to(pose1) (matching.py:204-207);
 * threshold: config guided_matching_threshold (radians).
 * Integer-valued stores rank the candidates by the exact integer distance; float stores (root-SIFT, feature_root) by the float32
 * distance in the oracle's accumulation order (oracle/guided_oracle.c l2sqr), read from the store's float rows.
 */
int osfm_match_pairs_guided(osfm_ctx *ctx, const osfm_store *store, const float *bearings, const int32_t *pairs, int64_t n_pairs,
                            const double *poses, double threshold, const osfm_match_params *params, const int32_t *cam_model_or_null,
                            const double *cam_params_or_null, const osfm_relpose_params *relpose_or_null, osfm_match_result **out,
                            osfm_match_timings *timings_or_null);

/* =====================================================================================
 * Bag-of-words side of pair matching and pair preselection.
 *
 * osfm_words_store / osfm_match_words_pairs  replace pyfeatures.match_using_words (opensfm/src/features/src/matching.cc:24-88) as
 *   matching.match_words / match_words_symmetric call it (opensfm/matching.py:637-680), for a whole pair list: descriptors
 *   (float32, total x 128) and the n closest vocabulary words of every feature (int32, total x words_per_feature, data.load_words)
 *   are uploaded once; per pair, every feature of one image checks the features of the other image filed under its words, in word
 *   order, stopping after the word that brings the count to max_checks; Lowe's test best < ratio * second in float; symmetric = the
 *   intersection of both directions.  counts[p] matches (i, j) of pair p land in matches[(p * max_count + k) * 2 ..], ordered by i
 *   (the reference returns them in set order, i.e. unspecified), max_count = osfm_words_store_max_count.
 * osfm_vlad_descriptor  replaces pyfeatures.compute_vlad_descriptor (matching.cc:93-124; the caller normalises, vlad.py);
 * osfm_vlad_distances   replaces the distance loop of compute_vlad_distances (matching.cc:126-152): L2 norms of reference - others[j];
 * osfm_knn_points / osfm_radius_points  replace spatial.cKDTree(points).query(point, k, distance_upper_bound) of
 *   match_candidates_by_distance (opensfm/pairs_selection.py:188-212): the k nearest candidates within max_distance in ascending
 *   distance (missing: index -1, distance inf), or -- when k covers every candidate -- the bit mask of the candidates within range.
 * ===================================================================================== */
typedef struct osfm_words_store osfm_words_store;
int osfm_words_store_create(osfm_ctx *ctx, int n_images, const int32_t *counts, int dim, int words_per_feature, const float *desc,
                            const int32_t *words, osfm_words_store **out);
void osfm_words_store_destroy(osfm_words_store *s);
int osfm_words_store_max_count(const osfm_words_store *s);
int osfm_match_words_pairs(osfm_ctx *ctx, const osfm_words_store *store, const int32_t *pairs, int64_t n_pairs, float lowes_ratio,
                           int max_checks, int symmetric, int32_t *counts, int32_t *matches, double *kernel_ms);
int osfm_vlad_descriptor(osfm_ctx *ctx, const float *features, int n, const float *centers, int n_centers, int dim, float *out);
int osfm_vlad_distances(osfm_ctx *ctx, const float *reference, const float *others, int m, int len, double *out);
/* pairs_selection.bow_distances (opensfm/pairs_selection.py:690-708): out[c] = np.fabs(reference - others[c]).sum() over float64 BoW
 * histograms (bow.py:34-36), in numpy's summation order (pairwise blocks of 128 with eight accumulators, 8192-element chunks). */
int osfm_bow_distances(osfm_ctx *ctx, const double *reference, const double *others, int m, int len, double *out);
int osfm_knn_points(osfm_ctx *ctx, const double *candidates, int n_candidates, const double *queries, int n_queries, int k,
                    double max_distance, double *out_distance, int32_t *out_index);
int osfm_radius_points(osfm_ctx *ctx, const double *candidates, int n_candidates, const double *queries, int n_queries,
                       double max_distance, uint32_t *out_mask);

/* =====================================================================================
 * HAHOG feature extraction
 *
 * osfm_hahog_extract replaces pyfeatures.hahog(image, peak_threshold, edge_threshold, target_num_features)
 * (opensfm/src/features/src/hahog.cc:125-206; binding opensfm/src/features/python/pybind.cc) together with the descriptor
 * post-processing of its only caller, features.extract_features_hahog (opensfm/features.py:516-534):
 *   image     rows x cols float32 grey levels in [0, 1] (host), at least 17 x 17
 *   points    n x 4: x, y, size, angle in degrees (hahog.cc:170-177);  desc  n x 128
 *   flags     OSFM_HAHOG_ROOT: square roots (feature_root);  OSFM_HAHOG_UCHAR: x 362 (x 512 without ROOT), clipped to [0, 255] and
 *             rounded (hahog_normalize_to_uchar) -- the integer-valued descriptors the matcher takes on its int8 path.  0: vlfeat's.
 *   capacity  rows available in points / desc; 4 x target_num_features always suffices (at most four orientations per feature).
 * Vlfeat's Hessian detector (covdet.c), the selection of the strongest features, orientations and SIFT descriptors (sift.c) are
 * followed operation for operation: the detected set, keypoints and descriptors are the reference's (tests/test_gpu_hahog.py states
 * the tolerance and what can differ).  target_num_features = 0 returns no features, as the reference does (hahog.cc:24-27 keeps
 * `target` of the sorted list).  OSFM_E_INVALID when the features do not fit `capacity` (*n_features says how many there are).
 * ===================================================================================== */
#define OSFM_HAHOG_ROOT 1
#define OSFM_HAHOG_UCHAR 2
int osfm_hahog_extract(osfm_ctx *ctx, const float *image, int rows, int cols, float peak_threshold, float edge_threshold,
                       int target_num_features, int flags, float *points, float *desc, int capacity, int *n_features);
/* The same for a list of images (what `opensfm detect_features` runs over a data set, one image per process in the reference:
 * opensfm/actions/detect_features.py -> features_processing.run_features_processing): up to `concurrency` (0: 4; at most 16) images in
 * flight, each on its own HIP stream and host thread, so that the ~130 short launches and the two host round trips of one image run
 * underneath the kernels of the others.  images[i] is rows[i] x cols[i]; points[i] / desc[i] have capacities[i] rows; n_features[i] as
 * above.  Results are those of osfm_hahog_extract image by image.  OSFM_HAHOG_IMAGE_ON_DEVICE: the image pointers are device memory
 * (extraction from frames that are already resident, no host-to-device copy inside the call). */
#define OSFM_HAHOG_IMAGE_ON_DEVICE 4
/* OSFM_HAHOG_IMAGE_U8 (both entry points): the image pointers address uint8 grey levels 0 .. 255 (rows x cols bytes) instead of float32
 * in [0, 1]; the library forms level / 255 in float32 on the device -- what features.extract_features_hahog (opensfm/features.py:524)
 * does on the host before the call: identical features, a quarter of the bytes over PCIe and no host-side conversion pass. */
#define OSFM_HAHOG_IMAGE_U8 8
int osfm_hahog_extract_batch(osfm_ctx *ctx, int n_images, const float *const *images, const int *rows, const int *cols, float peak_threshold,
                             float edge_threshold, int target_num_features, int flags, float *const *points, float *const *desc,
                             const int *capacities, int *n_features, int concurrency);

/* =====================================================================================
 * Culling of the final point cloud (opensfm/reconstruction.py:1590-1594 -> sfm/src/map_helpers.cc), cloud.hip
 *
 * osfm_points_conditioning  restates FilterBadlyConditionedPoints (map_helpers.cc:20-164) with ComputePointInverseCovariance
 *   (geometry/src/covariance.cc):
 *   points      n_points x 3;  shot_pose  n_shots x 12: R (row-major) then t of the WORLD-TO-CAMERA pose of every shot, already composed
 *               with its rig;  shot_camera  n_shots indices into the camera table cam_model (n_cams) / cam_params (n_cams x 16, the
 *               layout listed at the OSFM_CAMERA_* definitions; all ten models);  obs_shot / obs_point  n_obs, in any order.
 *   Per landmark, over its observations in ascending input order: kept only if some pair of rays normalize(X - origin) has
 *   AngleBetweenVectors (triangulation.cc:66-73) > min_angle_deg * pi / 180 (strict; a NaN angle, 0 or 1 observations do not keep it);
 *   H = sum J^T J with J the 2 x 3 derivative of the projection with respect to the world point; rejected when H is not finite, when
 *   det H is not finite or |det H| < min_abs_det, when the smallest eigenvalue of H is <= 0 or not finite; otherwise
 *   cond = min(sqrt(lambda_max / lambda_min), 1000) (the eigenvalues of H itself, cyclic Jacobi: the ratio the reference takes from
 *   H^-1).  Then, sequentially in landmark order on the host: threshold = mean + 1.0 * population sigma of the surviving cond values,
 *   and every landmark with cond > threshold is removed.
 *   cond     n_points: NaN where rejected before the threshold;
 *   reason   n_points: 0 kept, 1 ray angle, 2 H not finite, 3 determinant, 4 eigenvalues, 5 above the threshold;
 *   threshold  NaN when no landmark reached the statistics;  n_removed  landmarks with reason != 0.
 *   min_angle_deg must lie in [0, 180].  No floating-point atomics: two runs are bit-equal.
 *
 * osfm_points_isolation  restates RemoveIsolatedPoints (map_helpers.cc:166-231): the positions cast to float32; per point the k + 1
 *   smallest squared L2 distances to all points (itself included) in float32 as ((dx*dx) + dy*dy) + dz*dz without contraction, the
 *   smallest dropped, the other k summed in ascending order in float64 and divided by k; threshold = mean + 1.25 * population sigma
 *   of these averages (sequentially in input order); removed[i] = avg[i] > threshold.  The search is exact (uniform grid, rings of
 *   cells, brute force for the queries the rings do not settle).  The grid does not span the bounding box but the 2 % .. 98 % quantile
 *   box of every axis (six selections over n floats on the host before the kernels); points outside it are clamped into the border
 *   cells, which keeps the result exact and keeps a few far points from stretching the cells.  Limits: a cloud with more than 2 % of
 *   its points far out on one side of an axis stretches the cells along it anyway, and a cloud whose bulk sits in a few cells of that
 *   box degrades towards all-pairs inside them -- both exact, both slow at scale.  n_points <= k removes nothing, as the reference does (avg and
 *   threshold NaN: nothing was computed).  1 <= k <= 31, and every coordinate must be finite as a float32 -- the reference's
 *   behaviour on non-finite coordinates is undefined: OSFM_E_INVALID otherwise.
 *
 * kernel_ms (both, may be NULL): device time of the kernels.  n_points == 0 / n_obs == 0 return without a launch.
 * ===================================================================================== */
int osfm_points_conditioning(osfm_ctx *ctx, const double *points, int n_points, const double *shot_pose, const int32_t *shot_camera, int n_shots,
                             const int32_t *cam_model, const double *cam_params, int n_cams, const int32_t *obs_shot, const int32_t *obs_point,
                             int64_t n_obs, double min_angle_deg, double min_abs_det, double *cond, uint8_t *reason, double *threshold,
                             int *n_removed, double *kernel_ms);
int osfm_points_isolation(osfm_ctx *ctx, const double *points, int n_points, int k, double *avg, uint8_t *removed, double *threshold,
                          int *n_removed, double *kernel_ms);

/* =====================================================================================
 * Triangulation of tracks (opensfm/reconstruction.py:1032-1073 TrackTriangulator.triangulate, `triangulation_type: FULL`), triangulate.hip
 *
 * Per track, over its observations in input order: fewer than 2 -> status 1.  TriangulateBearingsMidpoint (geometry/src/triangulation.cc:
 * 139-178): some pair (i, j < i) must have AngleBetweenVectors (through acos; 0 when |cos| >= 1) in [min_angle, pi - min_angle], else
 * status 2; the midpoint X = (I + BBt Cinv) A / n - Cinv BBtA; per observation in order, AngleBetweenVectors(X - o_i, w_i) > threshold
 * -> status 3, then (X - o_i) . w_i < min_depth -> status 4 (these very comparisons: a NaN angle passes).  A valid midpoint goes through
 * PointRefinement (triangulation.cc:221-233: Ceres' TinySolver, max_num_iterations = refinement_iterations, restated in
 * triangulate_core.h) and its result is stored without a further test -- with ONE divergence: a midpoint or a refined point that is
 * not finite is status 5, where the reference would store the NaN point (with finite input that takes min_angle_deg = 0 and parallel
 * rays).
 *   status           n_tracks: 0 triangulated, 1 fewer than 2 observations, 2 ray angle, 3 reprojection angle, 4 depth, 5 not finite;
 *   points           n_tracks x 3: NaN unless the status is 0;
 *   iterations_used  n_tracks: TinySolver's summary.iterations (0 unless the status is 0 or 5);  kernel_ms may be NULL.
 * Track t owns rows track_offsets[t] : track_offsets[t + 1] (n_tracks + 1 offsets, the first 0, non-decreasing).
 * osfm_triangulate_bearings  centers / bearings: the origins and bearings of the rows, already in world coordinates.
 * osfm_triangulate_tracks    obs_shot / obs_xy (normalised image coordinates) per row; shot_pose, shot_camera, cam_model, cam_params as
 *   for osfm_points_conditioning.  The kernel computes b = pixel_bearing, w = R^T b and o = -R^T t as it loads a row.
 * OSFM_E_INVALID: offsets that decrease or do not start at 0, a shot or camera index out of range, a non-finite observation or a
 * non-finite pose used by one (found by the kernel as it loads the rows), refinement_iterations < 0, min_angle_deg outside [0, 180].
 * n_tracks == 0 returns without a launch.  Every sum runs in an order fixed by the track's length alone, without floating-point
 * atomics: two runs are bit-equal.
 * ===================================================================================== */
typedef struct osfm_triangulate_params {
  double threshold;              /* triangulation_threshold: radians */
  double min_angle_deg;          /* triangulation_min_ray_angle */
  double min_depth;              /* triangulation_min_depth */
  int32_t refinement_iterations; /* triangulation_refinement_iterations */
  int32_t pad;
} osfm_triangulate_params;
/* the values of opensfm/config.py: 0.006, 1.0, 0.001, 10 */
void osfm_triangulate_params_default(osfm_triangulate_params *p);
int osfm_triangulate_bearings(osfm_ctx *ctx, const double *centers, const double *bearings, const int64_t *track_offsets, int n_tracks,
                              const osfm_triangulate_params *params, double *points, uint8_t *status, int32_t *iterations_used, double *kernel_ms);
/* PointRefinement alone (pygeometry.point_refinement for a batch): every track's `initial` point (n_tracks x 3) goes through the solver
 * over the track's rows and the result is stored as it is, without any test -- also for tracks of 0 or 1 rows. */
int osfm_triangulate_refine(osfm_ctx *ctx, const double *centers, const double *bearings, const int64_t *track_offsets, int n_tracks,
                            const double *initial, int refinement_iterations, double *points, int32_t *iterations_used, double *kernel_ms);
int osfm_triangulate_tracks(osfm_ctx *ctx, const double *shot_pose, const int32_t *shot_camera, int n_shots, const int32_t *cam_model,
                            const double *cam_params, int n_cams, const int32_t *obs_shot, const double *obs_xy, const int64_t *track_offsets,
                            int n_tracks, const osfm_triangulate_params *params, double *points, uint8_t *status, int32_t *iterations_used,
                            double *kernel_ms);

/* =====================================================================================
 * Robust triangulation of tracks (opensfm/reconstruction.py:922-1030 TrackTriangulator.triangulate_robust, `triangulation_type: ROBUST`),
 * triangulate.hip + triangulate_robust.h: per-track RANSAC over pairs of observations, every track of the batch in one call.
 *
 * Per track of n observations in input order (restated literally, the reference's quirks included): n < 2 -> status 1.  C = n (n - 1) / 2
 * pairs (i < j) in lexicographic order; up to 11 tries, each consuming one uniform draw u:
 *   id = (int64)(u * (double)(C - 1))  (the last pair is never drawn unless C == 1); an id an earlier try drew costs the try only;
 *   TriangulateBearingsMidpoint on the rows (i, j) of rank id alone (the pair test, the midpoint and the two per-row tests of the FULL
 *   path, with threshold, min_angle_deg, min_depth); invalid ends the try; X = PointRefinement(the two rows, midpoint);
 *   inliers of X over all rows: |(X - o_k) / |X - o_k| - w_k| < threshold (a chord, strict);
 *   only if there are more than the best so far: new_X = PointRefinement(inlier rows, X); ls_inliers of new_X over all rows; the best is
 *   (ls_inliers, new_X) if strictly more than the inliers, else (inliers, X); ratio = |best| / n; stop if ratio == 1, else stop if
 *   log(1 - 0.99) / log(1 - ratio^2) <= i, i being the FIRST INDEX OF THE SAMPLED PAIR (the reference's loop variable is shadowed).
 * A best of more than one inlier is the point (status 0) and exactly the best inliers observe it; otherwise status 6.  One divergence,
 * that of the FULL path: a best point that is not finite is status 5.
 *   status       n_tracks: 0 triangulated, 1 fewer than 2 observations, 5 not finite, 6 no consensus (no valid sample, or a best of
 *                fewer than 2 inliers);
 *   points       n_tracks x 3: NaN unless the status is 0;
 *   inlier_mask  one byte per observation row: 1 for the best inliers of a track of status 0, else 0;
 *   n_inliers    n_tracks: the number of those (0 unless the status is 0);
 *   tries_used   n_tracks: draws consumed (tries made, repeats included; 0 for status 1);  kernel_ms may be NULL.
 * Randomness: track t owns 11 draws and never depends on another track or on the grid.  `draws` is n_tracks x 11 values in [0, 1) (a
 * value outside, or not finite: OSFM_E_INVALID, found by the kernel), or NULL: draw k of track t is then, in uint64 arithmetic,
 *   z = seed + 0x9E3779B97F4A7C15 * (11 t + k + 1);  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *   z = z ^ (z >> 31);  u = (double)(z >> 11) * 2^-53
 * (splitmix64's finaliser).  The distribution is the reference's; the stream is not numpy's global generator and cannot be -- the
 * number of draws the reference consumes per track depends on the outcome of the tracks before it.
 * Arguments, errors and the order of sums are those of the FULL calls above: two runs are bit-equal.
 * ===================================================================================== */
int osfm_triangulate_bearings_robust(osfm_ctx *ctx, const double *centers, const double *bearings, const int64_t *track_offsets, int n_tracks,
                                     const osfm_triangulate_params *params, const double *draws, uint64_t seed, double *points, uint8_t *status,
                                     uint8_t *inlier_mask, int32_t *n_inliers, int32_t *tries_used, double *kernel_ms);
int osfm_triangulate_tracks_robust(osfm_ctx *ctx, const double *shot_pose, const int32_t *shot_camera, int n_shots, const int32_t *cam_model,
                                   const double *cam_params, int n_cams, const int32_t *obs_shot, const double *obs_xy,
                                   const int64_t *track_offsets, int n_tracks, const osfm_triangulate_params *params, const double *draws,
                                   uint64_t seed, double *points, uint8_t *status, uint8_t *inlier_mask, int32_t *n_inliers,
                                   int32_t *tries_used, double *kernel_ms);

/* =====================================================================================
 * Depthmaps (opensfm/src/dense/src/depthmap.cc: dense::DepthmapEstimator and dense::DepthmapCleaner), depthmap.hip + depthmap_core.h:
 * what dense.compute_depthmap and dense.clean_depthmap do shot by shot, for a batch of shots in one call.
 *
 * OpenCV is not available to this project, so depthmap.cc is RESTATED, quirks included: float32 where it uses float, double where it
 * uses double, its order of operations, no contraction.  Per candidate plane v and other view o:  H = K_o (Q_o + a_o v^T) K_0^-1 in
 * double (Q_o = R_o R_0^T, a_o = Q_o t_0 - t_o, every product summed k = 0, 1, 2), narrowed to float; u, v, w, the four derivatives and
 * the sample coordinates of lines 433-459; LinearInterpolation is 0 outside [0, cols - 1) x [0, rows - 1); the six NCC sums accumulate
 * in float, dy then dx; the score is -1 when the weights sum to 0 or a variance is below 0.1; over the views a strict > keeps the lowest
 * view index on a tie.  BRUTE_FORCE: plane d has the depth of lines 193-198 and the normal (0, 0, -1); a candidate is accepted only if
 * its score exceeds the current one, starting from 0, so a pixel whose NCC is never positive stays all-zero.  PATCH_MATCH and
 * PATCH_MATCH_SAMPLE: RandomInitialization, ComputeIgnoreMask (mask == 0, or the population variance of the patch, in float, below
 * min_patch_sd^2), patchmatch_iterations forward and backward raster sweeps -- two adjacent-plane candidates, six perturbations with
 * the ranges 0.02 * 0.3^k and 0.5 * 0.8^k, in sample mode with more than two views one other-neighbour candidate, each using the current
 * values -- and PostProcess (5 x 5 median, depth zeroed where depth == 0 or |d - m| / d > 0.05).  The sweeps run as diagonal
 * wavefronts, which reproduce the sequential raster order exactly.  DepthmapCleaner::Clean is lines 515-541: the backprojected point and
 * the reprojection narrowed to float, the z_epsilon and NaN tests, |depth_at - depth_of| < depth_of * same_depth_threshold.
 * From memory of OpenCV, NOT compared with its source: the 3 x 3 inverse (cofactors times the reciprocal determinant), Vec3f / float as a
 * product with 1.f / alpha, and cv::medianBlur's replicated border.  Whether the unqualified exp() (lines 344, 473) and fabs() (line 485) resolve to the float or
 * the double overload is not pinned either; a refused call has touched none of the caller's outputs.
 * Divergences:
 *   - a sample coordinate that is NaN reads as 0 (the reference casts it to int: undefined);
 *   - the bilateral weight: its argument in float as at line 473, exp() in double on the host, rounded to float, tabulated by |dcolor|
 *     (0 .. 255) and dx^2 + dy^2 (0 .. 98) -- within one float ulp of the reference's expf;
 *   - randomness (the reference draws from rand() and a random_device-seeded mt19937: two of its own runs differ).  Draw k of pixel
 *     `pixel` = row * width + column in sweep s (0 the initialisation, 1 + 2 it / 2 + 2 it the forward / backward pass of iteration it) is,
 *     in uint64 arithmetic,  z = seed + 0x9E3779B97F4A7C15 * (((s << 40) + pixel) * 32 + k + 1), then splitmix64's finaliser (as for
 *     robust triangulation).  Initialisation: k = 0 depth = init_depth[z >> 52], k = 1, 2 normal x, y = (float)(z >> 40) * 2^-23 - 1,
 *     k = 3 neighbour = 1 + (uint32)(z >> 32) mod (N - 1).  A sweep: perturbation q uses k = 3 q for the depth factor
 *     factor[q][z >> 52] and k = 3 q + 1, 3 q + 2 for normal[z >> 52]; k = 18 is the other neighbour
 *     1 + (current + (uint32)(z >> 32) mod (N - 2)) mod (N - 1)  (an offset instead of the reference's redraw loop).  The tables are
 *     built on the host in double: normal[m] = Phi^-1((m + 1/2) / 4096), factor[q][m] = exp(depth_range_q * normal[m]),
 *     init_depth[m] = exp(log min + (log max - log min) (m + 1/2) / 4096).  Same distributions, discretised; another mechanism;
 *   - an even patch_size (the reference's Variance then reads stale buffer entries) and patch_size 1 (its sweep reads outside the image)
 *     are refused; with a single view no candidate is ever scored in a view: both PatchMatch modes keep the initial score -1 and
 *     nghbr 0 (the reference's sample mode scores view 0 against itself), brute force stays all-zero as in the reference.
 * A batch: problem b owns the views view_offsets[b] .. view_offsets[b + 1] (at most 32; none: nothing is written), the first being the
 * shot itself.  K, R (row-major 3 x 3) and t per view; images / masks / depths are per-view pointers to row-major height x width
 * arrays (only the mask of a problem's first view is read); views may differ in size.  Outputs are per-problem pointers to the shot's
 * height x width arrays: depth, plane (x 3), score float32 and nghbr int32.  An image smaller than the patch gives zeros without a
 * launch.  OSFM_E_INVALID: an even patch_size, one below 3 or above 15, more than 32 views, a K, R or t that is not finite,
 * min_depth <= 0 or max_depth < min_depth (estimate), num_depth_planes < 1.  A batch gives byte for byte what single calls give, and
 * two runs are byte-equal.  kernel_ms may be NULL.
 * osfm_depthmap_tables copies the tables the library uses: normal (4096), factor (6 x 4096), weight (256 x 99) and, for a depth range,
 * init_depth (4096); any pointer may be NULL.
 * ===================================================================================== */
#define OSFM_DEPTHMAP_BRUTE_FORCE 0
#define OSFM_DEPTHMAP_PATCH_MATCH 1
#define OSFM_DEPTHMAP_PATCH_MATCH_SAMPLE 2
typedef struct osfm_depthmap_params { /* opensfm/config.py:346-368 */
  double min_depth;             /* depthmap_min_depth: 0 = inferred by the caller */
  double max_depth;             /* depthmap_max_depth */
  double min_patch_sd;          /* depthmap_min_patch_sd */
  double min_correlation_score; /* depthmap_min_correlation_score (applied by the Python layer, as dense.compute_depthmap does) */
  double same_depth_threshold;  /* depthmap_same_depth_threshold */
  int32_t method;               /* depthmap_method: OSFM_DEPTHMAP_* */
  int32_t resolution;           /* depthmap_resolution */
  int32_t num_neighbors;        /* depthmap_num_neighbors */
  int32_t num_matching_views;   /* depthmap_num_matching_views */
  int32_t patchmatch_iterations;
  int32_t patch_size;
  int32_t min_consistent_views;
  int32_t num_depth_planes;     /* 100: what dense.compute_depthmap passes to set_depth_range */
  int32_t pad;
} osfm_depthmap_params;

void osfm_depthmap_params_default(osfm_depthmap_params *p);
int osfm_depthmap_tables(double min_depth, double max_depth, float *normal, float *factor, float *weight, float *init_depth);
int osfm_depthmap_estimate(osfm_ctx *ctx, int n_problems, const int32_t *view_offsets, const double *K, const double *R, const double *t,
                           const uint8_t *const *images, const uint8_t *const *masks, const int32_t *widths, const int32_t *heights,
                           const double *min_depth, const double *max_depth, const osfm_depthmap_params *params, uint64_t seed,
                           float *const *depth, float *const *plane, float *const *score, int32_t *const *nghbr, double *kernel_ms);
int osfm_depthmap_clean(osfm_ctx *ctx, int n_problems, const int32_t *view_offsets, const double *K, const double *R, const double *t,
                        const float *const *depths, const int32_t *widths, const int32_t *heights, const osfm_depthmap_params *params,
                        float *const *clean, double *kernel_ms);

/* -------------------------------------------------------------------------------------
 * Pruning and merging (dense::DepthmapPruner::Prune, depthmap.cc:565-625), prune.hip + prune_core.h: what dense.prune_depthmap does
 * shot by shot and dense.merge_depthmaps concatenates, for a batch of shots in one call.  The pruner does not stay on the host: its
 * raster-ordered push_back is a prefix sum over per-pixel keep flags.
 *
 * RESTATED like the cleaner, with the pruner's own types.  Pixel (i, j) of a problem's first view: depth <= 0 skips it (a NaN depth
 * does not: the pixel then meets only skipped views and is kept with a NaN point); normal = cv::normalize(plane);
 * area = (float)((double)(-normal_z / depth) * K0(0,0)); point = Backproject in double narrowed to float.  Per other view the point is
 * widened and projected in DOUBLE; the view is skipped when z < 1e-8 or z is NaN; iu = (int64)(x / z + 0.5), iv likewise -- truncation
 * toward zero, so a value in (-1, 0) lands on column or row 0 and counts as inside; outside the image the view is skipped;
 * depth_at = depths[other](iv, iu); when depth_at > (double)(1.f - (float)same_depth_threshold) * z the pixel is rejected if
 * depth_at == 0 (reachable with a threshold of 1 or more) or if (double)(-normalize(planes[other](iv, iu))_z / depth_at) * Ko(0,0) > area.
 * A kept pixel gives one row: the point, Rinv * normal (Rinv = R0 transposed, narrowed to float; float products summed k = 0, 1, 2),
 * the colour and the label of view 0.
 * From memory of OpenCV, NOT compared with its source: cv::normalize(Vec3f) as nv = sqrt of the squares summed in double, k = 0, 1, 2,
 * then v * (nv ? 1. / nv : 0.) with each product formed in double and rounded to float; the order of the Matx33f * Vec3f sums.
 * Divergences, both in place of undefined or implementation-defined behaviour:
 *   1. x / z + 0.5 (or y / z + 0.5) that is NaN, infinite or 2^31 or more in magnitude counts as outside the image (the reference casts
 *      it to int64: undefined);
 *   2. the reference passes that int64 to IsInsideImage(..., int, int), an implementation-defined narrowing: the same values count as
 *      outside here.
 * The batch is laid out as for osfm_depthmap_clean; depths[v] is height x width float32, planes[v] height x width x 3 float32; colors[v]
 * (height x width x 3) and labels[v] (height x width) are read, and uploaded, for the FIRST view of a problem only and may be NULL for
 * the others.  The outputs are the merged cloud of the batch: the rows of problem 0 in raster order, then those of problem 1, ...;
 * counts[b] (n_problems entries) gives the split.  A problem with no views or an empty first view has no rows.  `capacity` is the number
 * of rows points (x 3), normals (x 3), out_colors (x 3) and out_labels hold: a batch that keeps more fails with OSFM_E_INVALID, counts
 * filled in and the four outputs untouched (the number of first-view pixels with depth > 0 or NaN is always enough).  OSFM_E_INVALID
 * also: a NaN same_depth_threshold, more than 32 views, a K, R or t that is not finite.  Zero problems: OSFM_OK, nothing launched.
 * No atomic decides a row's place: a batch gives byte for byte what its single calls give, and two runs are byte-equal.  kernel_ms (may
 * be NULL) is the sum of the three kernels; osfm_depthmap_prune_split_ms gives ms[3] = mark, scan, scatter of the context's last call
 * that launched them.
 * ------------------------------------------------------------------------------------- */
int osfm_depthmap_prune(osfm_ctx *ctx, int n_problems, const int32_t *view_offsets, const double *K, const double *R, const double *t,
                        const float *const *depths, const float *const *planes, const uint8_t *const *colors, const uint8_t *const *labels,
                        const int32_t *widths, const int32_t *heights, const osfm_depthmap_params *params, int64_t capacity, float *points,
                        float *normals, uint8_t *out_colors, uint8_t *out_labels, int64_t *counts /* n_problems */, double *kernel_ms);
int osfm_depthmap_prune_split_ms(osfm_ctx *ctx, double *ms /* 3 */);

/* =====================================================================================
 * Image undistortion (opensfm/undistort.py: undistort_image, scale_image, render_perspective_view_of_a_panorama), a batch per call.
 *
 * osfm_camera_mapping is pygeometry.compute_camera_mapping (geometry/src/camera.cc:319-342) literally, in double, without contraction:
 * n = max(width, height), uv = (u - width 0.5, v - height 0.5), p = n from.Project(to.Bearing((1 / n) uv)),
 * map1[v][u] = (float)(p0 + width 0.5), map2[v][u] = (float)(p1 + height 0.5); the bearing is the normalised one of osfm_pixel_bearings.
 * Entry i has its own (from, to, width, height): cameras as model id + 16 doubles in the native order.  map1[i] / map2[i] point to
 * height x width floats.  osfm_panorama_mapping is the map of render_perspective_view_of_a_panorama: destination pixel (float32) ->
 * normalized_image_coordinates (float32 arithmetic, as numpy does there) -> the bearing of the view camera `to` -> rotations[i]
 * (R_pano R_view^T, row-major 3 x 3) -> from.Project -> denormalized_image_coordinates for a src_w x src_h panorama, narrowed to float.
 *
 * OpenCV is not available to this project, so cv2.remap and cv2.resize are RESTATED from memory of OpenCV, unpinned:
 *   - OSFM_INTER_LINEAR on uint8 (OSFM_INTER_AREA is treated as OSFM_INTER_LINEAR, as cv2.remap does): sx = round_half_even(x 32),
 *     integer part sx >> 5 (arithmetic shift: floor), fraction fx = sx & 31, the same for y; the four taps get the int32 weights
 *     32 (32 - fx)(32 - fy), 32 fx (32 - fy), 32 (32 - fx) fy, 32 fx fy (their sum is 32768); out = (sum tap weight + 16384) >> 15,
 *     per channel with the same weights;
 *   - OSFM_INTER_NEAREST: the tap (round_half_even(x), round_half_even(y));
 *   - OSFM_BORDER_CONSTANT: a tap outside the image reads 0;  OSFM_BORDER_WRAP: a tap index is taken modulo the size in both axes, with a
 *     non-negative result;
 *   - out_w == map_w and out_h == map_h: no scaling.  Anything else is scale_image's cv2.resize(INTER_NEAREST) of the full-size remap:
 *     output pixel X reads the map at src_x = min(floor(X (1.0 / ((double)out_w / map_w))), map_w - 1), the same in y, and only those
 *     pixels are computed -- byte for byte what full-size remap followed by nearest resize gives.  The output size itself
 *     (int(round(w factor)) with Python's round) is the caller's.
 * Divergences:
 *   - a map entry that is NaN or infinite, or whose rounded fixed-point value does not fit int32, gives 0 in either border mode
 *     (OpenCV's cast is undefined there);
 *   - an image, map or output side above 32767 is refused (OpenCV's int16 maps cannot address it either);
 *   - only uint8 with 1, 3 or 4 interleaved channels; uint16 ("anydepth") images are refused by the Python layer with the code of
 *     OSFM_E_INVALID and a message naming the dtype, never converted.
 * osfm_remap_images: image i (src_w x src_h x channels) through map1[i] / map2[i] (map_w x map_h; images may share a map: it is uploaded
 * once) into dst[i] (out_w x out_h x channels).  osfm_undistort_images is the fused path for frame cameras: image i uses the pair
 * (from, to) number image_cam[i] of a table of n_cams pairs; the map entry is computed in registers by the function osfm_camera_mapping
 * uses and narrowed to float, so the bytes equal osfm_remap_images on osfm_camera_mapping's output; border OSFM_BORDER_CONSTANT.
 * A batch of zero is a no-op that succeeds; a batch holds at most 65535 entries.  OSFM_E_INVALID: channels not 1, 3 or 4, a non-positive
 * size, a side above 32767, a camera parameter (or rotation entry) that is not finite, an unknown model, interpolation or border value,
 * an image_cam index out of range; a refused call has touched none of the caller's outputs.  A batch gives byte for byte what single
 * calls give, and two runs are byte-equal.  kernel_ms may be NULL; it is written by calls that succeed (0 for an empty batch).
 * ===================================================================================== */
#define OSFM_INTER_NEAREST 0 /* cv2.INTER_NEAREST */
#define OSFM_INTER_LINEAR 1  /* cv2.INTER_LINEAR */
#define OSFM_INTER_AREA 3    /* cv2.INTER_AREA */
#define OSFM_BORDER_CONSTANT 0 /* cv2.BORDER_CONSTANT */
#define OSFM_BORDER_WRAP 3     /* cv2.BORDER_WRAP */
int osfm_camera_mapping(osfm_ctx *ctx, int n_maps, const int32_t *from_model, const double *from_params, const int32_t *to_model,
                        const double *to_params, const int32_t *widths, const int32_t *heights, float *const *map1, float *const *map2,
                        double *kernel_ms);
int osfm_panorama_mapping(osfm_ctx *ctx, int n_maps, const int32_t *from_model, const double *from_params, const int32_t *to_model,
                          const double *to_params, const double *rotations, const int32_t *src_w, const int32_t *src_h,
                          const int32_t *widths, const int32_t *heights, float *const *map1, float *const *map2, double *kernel_ms);
int osfm_remap_images(osfm_ctx *ctx, int n_images, const uint8_t *const *src, const int32_t *src_w, const int32_t *src_h,
                      const int32_t *channels, const float *const *map1, const float *const *map2, const int32_t *map_w,
                      const int32_t *map_h, const int32_t *out_w, const int32_t *out_h, int interpolation, int border, uint8_t *const *dst,
                      double *kernel_ms);
int osfm_undistort_images(osfm_ctx *ctx, int n_images, const uint8_t *const *src, const int32_t *widths, const int32_t *heights,
                          const int32_t *channels, const int32_t *image_cam, int n_cams, const int32_t *from_model, const double *from_params,
                          const int32_t *to_model, const double *to_params, const int32_t *out_w, const int32_t *out_h, int interpolation,
                          uint8_t *const *dst, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* OSFM_MI355_H */
