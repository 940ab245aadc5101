/*
 * msfl_c_api.h — C ABI of the MI355X-native LOAM scan-matching engine (libmsfl_hip.so).
 *
 * This is the drop-in boundary for the ONE hot path of kekeliu-whu/MSF_LOAM:
 *   stage A  per-scan feature extraction      reference src/msf_loam_node.cc:160-378
 *   stage B  scan-to-scan registration        reference src/slam/local/scan_matching/odometry_scan_matcher.cc:43-285
 *   stage C  scan-to-local-map registration   reference src/slam/local/scan_matching/mapping_scan_matcher.cc:19-278
 *
 * Plain C, plain pointers and sizes, no torch / PCL / Eigen / Ceres types. Every entry point
 * cites the reference interface it replaces.  A maintainer-side binding (C++ adapter with the
 * reference's own method signatures) is shown in INTEGRATION.md and shipped as
 * include/msfl_scan_matcher.hpp.
 *
 * Conventions
 *   - Points are 16-byte records {x, y, z, t}.  `t` is what the reference keeps in
 *     pcl::PointXYZI::intensity, i.e. the per-point relative time in seconds
 *     (msf_loam_node.cc:152-153 writes time into intensity).
 *   - A pose is 7 doubles [tx ty tz qx qy qz qw], the layout of Rigid3d::ToVector7()
 *     (src/common/rigid_transform.h:59-64).  Poses are IN/OUT: initial guess in, result out,
 *     exactly like the reference's `Rigid3d *pose_estimate` arguments.
 *   - Every pointer argument is tagged by a `mem` flag: MSFL_MEM_HOST (the library stages the
 *     copy) or MSFL_MEM_DEVICE (already resident in HBM on the handle's device; nothing is copied).
 *   - All functions return an msfl_status.  No exceptions, no aborts: the reference's glog CHECK
 *     failures and out-of-bounds reads (SURVEY.md §8b "edge cases") become status codes.
 *   - A handle owns one HIP stream and all device scratch.  Handles are independent, so the
 *     odometry thread and the mapping thread of the reference (laser_odometry.h:29,
 *     laser_mapping.h:65) each own one and may call concurrently.  A single handle is not
 *     re-entrant (neither is a reference matcher instance).
 */
#ifndef MSFL_C_API_H_
#define MSFL_C_API_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSFL_API_VERSION 1

typedef struct msfl_handle_s msfl_handle;

typedef enum msfl_status {
  MSFL_OK = 0,
  /* odometry_scan_matcher.cc:262-267 returns false when corner+plane correspondences < 10.
     Per-scan status in batched calls; the pose keeps the value of the last completed solve. */
  MSFL_TOO_FEW_CORRESPONDENCES = 1,
  /* mapping_scan_matcher.cc:128,198 index pointSearchSqDis[4] unguarded; the reference relies on
     the caller's gate (laser_mapping.cc:284-285).  Here: map cloud with < 5 points. */
  MSFL_MAP_TOO_SMALL = 2,
  MSFL_BAD_ARG = 3,
  MSFL_HIP_ERROR = 4,
  /* msf_loam_node.cc:136 CHECK_LT(point.ring, 128) / :186 CHECK_GT(valid_scan_num, 0) */
  MSFL_BAD_RING = 5,
  MSFL_NO_MAP = 6,
  MSFL_CAPACITY = 7
} msfl_status;

typedef enum msfl_mem { MSFL_MEM_HOST = 0, MSFL_MEM_DEVICE = 1 } msfl_mem;

/* 16-byte point: pcl::PointXYZI as the matchers see it (x,y,z + intensity==relative time). */
typedef struct msfl_point {
  float x, y, z, t;
} msfl_point;

/*
 * All hot-path thresholds of the reference are compile-time constants (SURVEY.md §8a
 * "Constants").  They are exposed as a POD with the reference values as defaults
 * (msfl_default_params).  Parity claims hold for the defaults.
 */
typedef struct msfl_params {
  /* --- stage A, msf_loam_node.cc --- */
  double scan_period;            /* kScanPeriod = 0.1                     :80      */
  double min_range;              /* g_min_range, launch default 0.3       :434     */
  float  curvature_threshold;    /* 0.1                                   :275,312 */
  float  neighbor_gap_sq;        /* 0.05                                  :293,300 */
  int    sectors_per_ring;       /* 6                                     :255     */
  int    max_sharp_per_sector;   /* 2                                     :277     */
  int    max_less_sharp_per_sector; /* 20                                 :281     */
  int    max_flat_per_sector;    /* 4                                     :317     */
  /* --- stage B, odometry_scan_matcher.cc:15-18 --- */
  double odom_distance_sq_threshold; /* kDistanceSqThreshold = 25 */
  double odom_nearby_scan;           /* kNearByScan = 2.5         */
  int    odom_min_correspondences;   /* 10, :262                  */
  /* --- stage C, mapping_scan_matcher.cc --- */
  int    map_knn;                /* 5 (fixed by the kernels; other values -> MSFL_BAD_ARG) :125 */
  float  map_knn_max_sq_dist;    /* 1.0   :128,198 */
  double line_eigen_ratio;       /* 3.0   :147     */
  double plane_tolerance;        /* 0.2   :216     */
  /* --- shared solver settings (both matchers) --- */
  int    outer_iterations;       /* kOptimalNum = 2, mapping_scan_matcher.cc:15 */
  int    max_lm_iterations;      /* options.max_num_iterations = 6, :252 */
  double huber_delta;            /* ceres::HuberLoss(0.1), :77 */
  /* Ceres Solver::Options defaults the reference leaves untouched (third party, not in tree). */
  double initial_trust_region_radius; /* 1e4   */
  double max_trust_region_radius;     /* 1e16  */
  double min_trust_region_radius;     /* 1e-32 */
  double min_relative_decrease;       /* 1e-3  */
  double min_lm_diagonal;             /* 1e-6  */
  double max_lm_diagonal;             /* 1e32  */
  double function_tolerance;          /* 1e-6  */
  double gradient_tolerance;          /* 1e-10 */
  double parameter_tolerance;         /* 1e-8  */
  int    max_consecutive_invalid_steps; /* 5 */
} msfl_params;

/* Per-registration diagnostics (what the reference only logs via glog / Ceres BriefReport). */
typedef struct msfl_match_info {
  int    status;             /* msfl_status of this scan */
  int    n_edge[2];          /* accepted edge correspondences, outer iteration 0 / 1  (corner_num :173) */
  int    n_plane[2];         /* accepted plane correspondences (surf_num :243) */
  int    lm_iterations[2];   /* trust-region iterations executed (<= max_lm_iterations) */
  int    lm_successful[2];   /* accepted steps */
  double initial_cost[2];    /* Ceres cost (1/2 sum rho) at entry of each solve */
  double final_cost[2];      /* cost at the returned pose */
} msfl_match_info;

/* Per-registration uncertainty of the returned pose (opt-in: msfl_set_uncertainty / msfl_slam_set_uncertainty).  The reference
   has nothing here: its odometry messages are geometry_msgs::PoseWithCovariance whose 36 covariance doubles stay zero.
   `covariance` is for UNIT-VARIANCE residuals, which is what ceres::Covariance returns: scale it by `sigma2` (the a-posteriori
   variance factor of this solve) or by the variance of your own sensor model before using it as a pose covariance.  Both
   matrices are in the solver's tangent space; the rotation block is BODY-frame (see `information`), so a consumer that wants
   fixed parent axes (ROS) rotates it first: msfl::CovarianceInParentFrame in include/msfl/scan_matcher.hpp. */
typedef struct msfl_match_uncertainty {
  double information[36];   /* row-major H = J^T J of the LAST solve's problem at the RETURNED pose, robustified as Ceres
                               evaluates it (rows scaled by sqrt(rho'), i.e. what ceres::Covariance would see); tangent order
                               [dt(3), dtheta(3)] of PoseLocalParameterization: t += dt (parent frame), q = q * dq(dtheta) (body frame) */
  double eigenvalues[6];    /* ascending */
  double eigenvectors[36];  /* row k = unit eigenvector of eigenvalues[k]; sign: its largest-magnitude component (lowest index on ties) is positive */
  double covariance[36];    /* sum over kept k of v_k v_k^T / lambda_k: inverse of H, pseudo-inverse when directions are dropped */
  double sigma2;            /* a-posteriori variance factor 2 * final_cost / (n_residuals - 6); 0 when n_residuals <= 6 */
  int n_residuals;          /* 3 * edges + planes of that solve */
  int n_degenerate;         /* eigenvalues below max(min_eigenvalue, 1e-14 * lambda_max): dropped from `covariance` */
  int valid;                /* 0: no solve ran for this registration (status != 0, empty problem, too few correspondences): record all zero */
  int reserved_;
} msfl_match_uncertainty;

/* Optional Gaussian prior on the pose of one registration (opt-in: msfl_set_pose_prior / msfl_slam_set_next_prior): one more
   6-row residual block of the solved problem, WITHOUT a loss function (docs/kernels/prior.md).  For the pose x = (t, q):
     qe = conj(q0) * q, negated when qe.w < 0;   e = [t - t0 ; 2 * qe.xyz];   r = L e;   cost 1/2 |r|^2
   and, in the tangent space of PoseLocalParameterization, J = L * blockdiag(I3, qe.w * I3 + skew(qe.xyz)).  The tangent order
   [dt(3), dtheta(3)] and the body-frame rotation block are those of msfl_match_uncertainty.information: a Cholesky factor
   (upper triangular R with R^T R = information, or any L with L^T L = the wanted information, any rank) of a previous
   `information` or of an inverse covariance goes in unchanged.  The prior is not a correspondence: the min_correspondences gate
   and the "no correspondence at all: pose untouched" rule do not see it.  A record whose 36 sqrt_information entries are all
   zero is skipped: that registration is bit-identical to one without a prior. */
typedef struct msfl_pose_prior {
  double pose[7];              /* prior mean (t0, q0): x y z, then the UNIT quaternion x y z w */
  double sqrt_information[36]; /* row-major 6 x 6 L; information = L^T L */
} msfl_pose_prior;

/* Per-solve record of the degeneracy-aware solve (opt-in: msfl_set_degeneracy / msfl_slam_set_degeneracy;
   docs/kernels/degeneracy.md).  Index = outer iteration, as in msfl_match_info: every solve of a registration decomposes the
   matrix H0 it enters with ({lidar rows, robustified} + the pose prior's block, if one is set) and holds the eigen-directions
   below the threshold at the guess. */
typedef struct msfl_degeneracy_record {
  double eigenvalues[2][6];    /* of H0 at that solve's entry pose, ascending */
  double eigenvectors[2][36];  /* row k = eigenvector k, tangent order [dt, dtheta], sign as in msfl_match_uncertainty */
  int n_held[2];               /* eigenvalues below max(min_eigenvalue, 1e-14 * lambda_max): the solve did not move along them */
  int valid[2];                /* 0: no solve ran, the slice is all zero */
} msfl_degeneracy_record;

/* Outlier rejection in front of the solve (opt-in: msfl_set_outlier_rejection / msfl_slam_set_outlier_rejection;
   docs/kernels/rejection.md).  The reference's hooks are RefineByRejectOutliersWithThreshold / ...WithFrac (scan_matcher.cc:13-76). */
enum { MSFL_REJECT_OFF = 0, MSFL_REJECT_THRESHOLD = 1, MSFL_REJECT_FRACTION = 2 };   /* msfl_outlier_rejection.mode */
enum { MSFL_REJECT_LAST_OUTER = 0, MSFL_REJECT_EVERY_OUTER = 1 };                    /* msfl_outlier_rejection.which */
typedef struct msfl_outlier_rejection {
  int mode;          /* MSFL_REJECT_OFF / _THRESHOLD / _FRACTION */
  double threshold;  /* THRESHOLD: a correspondence goes unless its loss-free residual norm is <= threshold (reference: 0.2) */
  double fraction;   /* FRACTION: the ceil(n * fraction) correspondences of a scan with the largest residual norm go; in [0, 1] */
  int which;         /* MSFL_REJECT_LAST_OUTER (the reference's choice): before the last outer iteration's solve only; _EVERY_OUTER */
} msfl_outlier_rejection;
/* Per-solve record of the rejection; index = outer iteration, as in msfl_match_info.  56 bytes. */
typedef struct msfl_rejection_record {
  int n_edge_in[2], n_plane_in[2];              /* correspondences entering the solve, before rejection */
  int n_edge_rejected[2], n_plane_rejected[2];  /* of them rejected */
  double cut_sq[2];  /* squared residual norm at the cut: threshold^2 (THRESHOLD), the smallest rejected one (FRACTION; NaN if that
                        one is not finite); 0 when nothing was rejected */
  int valid[2];      /* 0: rejection did not run in front of that solve, the slice is all zero */
} msfl_rejection_record;

/* Accumulated GPU time per kernel class, measured with HIP events on the handle's stream
   (enabled by msfl_set_timing).  Used by bench.py for the live roofline figure. */
typedef struct msfl_timing {
  int    launches_assoc;   double ms_assoc;     /* transform + exact 5-NN kernel      */
  int    launches_solve;   double ms_solve;     /* persistent LM + Huber solve kernel */
  int    launches_index;   double ms_index;     /* map grid index build (all kernels) */
  int    launches_extract; double ms_extract;   /* feature extraction (all kernels)   */
  int    launches_odom;    double ms_odom;      /* scan-to-scan association kernel    */
  int    launches_fit;     double ms_fit;       /* line / plane fit kernel            */
  unsigned long long knn_candidates;            /* map points whose distance the 5-NN kernel evaluated (mode 3 only): the launches of the
                                                   first outer iteration */
  unsigned long long knn_candidates_seeded;     /* the same for the launches of the second outer iteration */
  int    launches_assoc_seeded; double ms_assoc_seeded;   /* the second iteration's 5-NN launches alone (also part of launches_assoc / ms_assoc) */
} msfl_timing;

/* ------------------------------------------------------------------------------------------ */
/* lifecycle                                                                                  */
/* ------------------------------------------------------------------------------------------ */

/* Fill `p` with the reference constants listed above. */
void msfl_default_params(msfl_params* p);

int msfl_api_version(void);

/* Replaces construction of the matcher objects (laser_odometry.cc:56, laser_mapping.cc:42).
   `params` may be NULL (defaults).  `device` is the HIP device ordinal. */
msfl_status msfl_create(const msfl_params* params, int device, msfl_handle** out);
void msfl_destroy(msfl_handle* h);

/* Run all work of this handle on a caller-provided hipStream_t (e.g. torch's current stream).
   The value is used as is: NULL means HIP's null (legacy default) stream, which is what
   torch.cuda.current_stream().cuda_stream is unless the caller switched streams.
   msfl_reset_stream goes back to the handle's own (non-blocking) stream. */
msfl_status msfl_set_stream(msfl_handle* h, void* hip_stream);
msfl_status msfl_reset_stream(msfl_handle* h);
/* Block until everything queued by this handle has finished. */
msfl_status msfl_synchronize(msfl_handle* h);

const char* msfl_status_string(int status);
/* Human-readable detail of the last non-OK status on this handle ("" if none). */
const char* msfl_last_error(const msfl_handle* h);

/* enabled: 0 off; 1 every kernel class; 2 only the association (5-NN) kernel — two events per launch
   instead of two per class, for timing the dominant kernel inside a throughput measurement; 3 like 1, and the
   5-NN kernel additionally counts the candidates it evaluates (a counting instantiation: slower, for the
   "distance evaluations per second" figure only). */
msfl_status msfl_set_timing(msfl_handle* h, int enabled);
msfl_status msfl_get_timing(msfl_handle* h, msfl_timing* out, int reset);

/* Uncertainty output, off by default.  out == NULL turns it off.  Otherwise EVERY later matcher call on this handle
   (msfl_match_scan2map, _batch, both deskew forms, msfl_match_pairs_batch, msfl_solve_records, _deskew, msfl_match_scan2scan, _batch)
   writes one record per registration into out[0 .. n), in the call's order; a call with more registrations than `capacity`
   returns MSFL_CAPACITY before it stages or launches anything (poses untouched).  A registration whose per-scan status is not 0, or
   whose last solve had nothing to solve, gets an all-zero record (valid = 0); a call that itself fails writes nothing.
     mem == MSFL_MEM_DEVICE : `out` is a device pointer, the write is asynchronous on the handle's stream, nothing is synchronised;
     mem == MSFL_MEM_HOST   : the records are copied like `info` (the call synchronises).
   min_eigenvalue (>= 0): eigen-directions of the information matrix below it are counted in n_degenerate and left out of
   `covariance`.  Poses, statuses and `info` of every call are bit-identical with the feature on and off: one more kernel runs
   after the last solve and reads what the solve left behind. */
msfl_status msfl_set_uncertainty(msfl_handle* h, msfl_match_uncertainty* out, int capacity, msfl_mem mem, double min_eigenvalue);

/* Pose priors, off by default.  priors == NULL turns them off.  Otherwise priors[b] is part of the problem of registration b in
   EVERY solve (both outer iterations) of every later matcher call on this handle (the calls msfl_set_uncertainty lists); a call
   with more registrations than `count` returns MSFL_CAPACITY before it stages or launches anything (poses untouched).  The
   pointer is kept, not the records: they are read at each call.
     mem == MSFL_MEM_DEVICE : `priors` is a device pointer, read on the handle's stream at each call, nothing is synchronised;
                              a record with a non-finite entry gives that registration the status MSFL_BAD_ARG (pose untouched).
     mem == MSFL_MEM_HOST   : the records are copied at each call like the other host inputs; a non-finite entry makes the call
                              return MSFL_BAD_ARG (msfl_last_error names the entry) before anything is staged.
   initial_cost / final_cost of `info` include the prior's cost; n_edge / n_plane do not change.  With msfl_set_uncertainty on,
   `information` is the posterior one (lidar J^T J + the prior's, at the returned pose) and n_residuals counts the six prior rows.
   With the feature off, or for an all-zero record, every output is bit-identical to what it was without this call. */
msfl_status msfl_set_pose_prior(msfl_handle* h, const msfl_pose_prior* priors, int count, msfl_mem mem);

/* Degeneracy-aware solve (solution remapping after Zhang & Singh), off by default; enabled == 0 turns it off.  Otherwise every
   solve of every later matcher call on this handle (the calls msfl_set_uncertainty lists; each outer iteration is one solve)
   decomposes its entry matrix H0 and updates the pose only along the eigen-directions with
   lambda_k >= max(min_eigenvalue, 1e-14 * lambda_max); the others stay at the guess.  A solve with nothing held is bit-identical
   to the feature-off solve; with all six held the pose passes through (lm_iterations = lm_successful = 0, final_cost =
   initial_cost, status 0).  A pose prior (msfl_set_pose_prior) is part of H0, so it can make a direction observable.
   `out` may be NULL (the remapping still runs); otherwise one record per registration goes to out[0 .. n) with the memory kinds,
   the MSFL_CAPACITY rule and "a failing call writes nothing" of msfl_set_uncertainty.  MSFL_BAD_ARG for a negative or
   non-finite min_eigenvalue.  The uncertainty output keeps its meaning: the full information at the returned pose. */
msfl_status msfl_set_degeneracy(msfl_handle* h, int enabled, double min_eigenvalue, msfl_degeneracy_record* out, int capacity,
                                msfl_mem mem);

/* Outlier rejection, off by default; cfg == NULL or cfg->mode == MSFL_REJECT_OFF turns it off.  Otherwise, in every later matcher
   call on this handle (the calls msfl_set_uncertainty lists), the selected solves (cfg->which; msfl_solve_records has one solve,
   which both values select) are preceded by a pass over the scan's correspondences at the solve's entry pose, all on the device:
     s = |N x (R p + t - C)|^2 for an edge, (N.(R p + t) - N.C)^2 for a plane, in f64 and without the loss;
     THRESHOLD : a correspondence is rejected iff !(s <= threshold^2), so one with a non-finite s goes;
     FRACTION  : with n the scan's correspondences of both kinds, the k = ceil(n * fraction) of them with the largest s go (the
                 product in double: n = 100, fraction = 0.07 rejects 8).  Equal s: the higher index goes first, corner features
                 numbered before surf features; a non-finite s ranks above every finite one.
   A rejected correspondence is from there on one that association refused: n_edge / n_plane of msfl_match_info count the
   survivors, odom_min_correspondences and the empty-problem rule apply to the survivors, and the uncertainty record is the
   information of the survivors.  A scan whose status is not 0 is skipped.
   `out` may be NULL (rejection still runs); otherwise one record per registration goes to out[0 .. n) with the memory kinds,
   the MSFL_CAPACITY rule and "a failing call writes nothing" of msfl_set_uncertainty.  MSFL_BAD_ARG for an unknown mode or
   `which`, a negative or non-finite threshold, or a fraction outside [0, 1].  With the feature off nothing is launched, staged
   or allocated and every output is bit-identical to what it was without this call. */
msfl_status msfl_set_outlier_rejection(msfl_handle* h, const msfl_outlier_rejection* cfg, msfl_rejection_record* out, int capacity,
                                       msfl_mem mem);

/* ------------------------------------------------------------------------------------------ */
/* stage C — scan-to-local-map registration                                                   */
/*   replaces MappingScanMatcher::MatchScan2Map (mapping_scan_matcher.h:14-21, .cc:19-278),    */
/*   LiDAR-only branch (!is_initialized, .cc:96,123,168-171,193,238-241,271).                  */
/* ------------------------------------------------------------------------------------------ */

/* Replaces the two pcl::KdTreeFLANN::setInputCloud calls (mapping_scan_matcher.cc:66-73):
   uploads (if host) and spatially indexes cloud_map.cloud_corner_less_sharp /
   cloud_map.cloud_surf_less_flat.  The index is an exact-kNN uniform grid.
   The map stays resident until the next msfl_set_map on this handle. */
msfl_status msfl_set_map(msfl_handle* h,
                         const msfl_point* corner, int n_corner,
                         const msfl_point* surf, int n_surf,
                         msfl_mem mem);

/* One registration against the resident map.
     corner/surf : scan_curr.cloud_corner_less_sharp / cloud_surf_less_flat (already voxel
                   down-sampled by the caller, laser_mapping.cc:264-270), scan frame.
     pose_io     : pose_estimate_map_scan2world, Vector7, in = guess, out = result.
     info        : optional diagnostics.
   Returns MSFL_OK (the reference always returns true, .cc:277) or an error status; with zero
   accepted correspondences the pose is returned unchanged (Ceres solves an empty problem). */
msfl_status msfl_match_scan2map(msfl_handle* h,
                                const msfl_point* corner, int n_corner,
                                const msfl_point* surf, int n_surf,
                                double pose_io[7], msfl_match_info* info,
                                msfl_mem mem);

/* B independent registrations against the same resident map in one call (the shape the
   north-star batches: "many scans shard embarrassingly").
     corner, corner_off : concatenated corner features and B+1 prefix offsets (scan b owns
                          [corner_off[b], corner_off[b+1]) ); same for surf.
     poses_io           : B x 7 doubles, in/out.
     status             : B ints out (msfl_status per scan), may be NULL.
     info               : B msfl_match_info out, may be NULL (host memory only).
   With mem == MSFL_MEM_DEVICE all five arrays and poses_io/status are device pointers and the
   call is asynchronous on the handle's stream. */
msfl_status msfl_match_scan2map_batch(msfl_handle* h, int n_scans,
                                      const msfl_point* corner, const int* corner_off,
                                      const msfl_point* surf, const int* surf_off,
                                      double* poses_io, int* status, msfl_match_info* info,
                                      msfl_mem mem);

/* P independent (map, scan) PAIRS in one call: scan p is registered against map p only ("many map-submap pairs").  The
   reference analogue is one MatchScan2Map call per pair, each rebuilding both kd-trees (mapping_scan_matcher.cc:66-73;
   laser_mapping.cc:304-311).  Here the P maps are indexed together (one exact-kNN grid per pair inside one set of arrays,
   four launches + one scan per cloud kind whatever P is) and the P registrations run as one batch.
     map_corner, map_corner_off : the P corner map clouds concatenated + P+1 prefix offsets (HOST array, like every batch
                                  call); same for map_surf.
     corner / surf + offsets    : the P scans' (down-sampled) feature clouds, as in msfl_match_scan2map_batch.
     poses_io, status, info     : as there.  status[p] = MSFL_MAP_TOO_SMALL for a pair whose corner or surf map has fewer
                                  than 5 points (the pose guess passes through); the call itself still returns MSFL_OK.
   Results equal P calls of msfl_set_map + msfl_match_scan2map bit for bit.  With MSFL_MEM_DEVICE the clouds, poses_io and
   status are device pointers and the call is asynchronous.  The handle's resident single map (msfl_set_map) is replaced:
   call msfl_set_map again before the next msfl_match_scan2map*.  The call is msfl_set_pair_maps followed by
   msfl_match_pairs_resident (below), and its pair index stays resident like theirs. */
msfl_status msfl_match_pairs_batch(msfl_handle* h, int n_pairs,
                                   const msfl_point* map_corner, const int* map_corner_off,
                                   const msfl_point* map_surf, const int* map_surf_off,
                                   const msfl_point* corner, const int* corner_off,
                                   const msfl_point* surf, const int* surf_off,
                                   double* poses_io, int* status, msfl_match_info* info, msfl_mem mem);

/* Fitness of a scan at given poses against the resident map, independent of any solve (the role of PCL's
   getFitnessScore): for every pose and every feature, the nearest map point OF THE FEATURE'S KIND (corner features
   query the corner map, surf features the surf map) within max_dist of the transformed feature, exactly: f32 transform
   and f32 squared distance as in the matcher, ties resolved to the lowest original map index.  A feature is an inlier
   when that squared distance d2 satisfies d2 <= (float)(max_dist * max_dist).  Sums are kept in fixed point, so a record
   is bit-reproducible whatever the call's shape: use it to grade a registration, to verify a candidate pose (a loop
   closure, a GPS fix, a result of msfl_match_pairs_batch) or to rank many hypotheses for one scan. */
typedef struct msfl_pose_score {
  int inliers[2];                     /* corner, surf features with a map point of their kind within max_dist */
  unsigned long long sum_sq_q32[2];   /* sum over those of rint(d2 * 2^32): squared metres in units of 2^-32 */
  int status;                         /* 0, or MSFL_BAD_ARG for a pose with a non-finite entry (record otherwise zero) */
  int reserved_;
} msfl_pose_score;

/* Scores one scan at n_poses poses (msfl_score_poses) or scan b of n_scans at the poses [pose_off[b], pose_off[b+1])
   (msfl_score_poses_batch; scores[i] belongs to poses[7*i .. 7*i+6]).
     corner/surf (+ offsets) : the scan's feature clouds as in msfl_match_scan2map(_batch), scan frame.
     poses                   : 7 doubles each (t, q xyzw), scan -> map.
     d2_out, nn_out          : optional (NULL: not wanted), n_poses x (n_corner + n_surf) values, row h = pose h, corner
                               features first: the squared distance and the ORIGINAL index (position in the cloud given to
                               msfl_set_map) of the nearest map point; +inf and -1 when none lies within max_dist, or when
                               the feature or its transformed point is not finite.
   Rules:
     - MSFL_NO_MAP without a resident single map, which includes the state after msfl_match_pairs_batch.
     - MSFL_BAD_ARG unless 0 < max_dist, max_dist^2 <= params.map_knn_max_sq_dist (the index is only exact up to the radius
       it was built for) and max_dist^2 <= 64 (the sum of any scan of fewer than 2^24 features then stays below 2^63); a NaN
       max_dist is MSFL_BAD_ARG.  A scan of 2^24 features or more is MSFL_CAPACITY.
     - Offset arrays are HOST arrays (n_scans + 1 prefix offsets each), like in every batch call.
     - With MSFL_MEM_DEVICE the clouds, poses, scores and d2_out / nn_out are device pointers and the call is asynchronous
       on the handle's stream, ordered after a preceding asynchronous msfl_set_map.
     - A map side without points gives zero inliers of that kind, not an error (no MSFL_MAP_TOO_SMALL here).
     - A pose with a non-finite entry gets status MSFL_BAD_ARG and an otherwise zero record (its d2_out / nn_out rows are
       +inf / -1); the call still returns MSFL_OK and the other poses are unaffected.
     - Any number of poses: more than fit one launch are served by several.
     - The call uses scratch of its own and never touches poses, records, neighbour lists or the index: a matcher call
       after it is bit-identical to one without it. */
msfl_status msfl_score_poses(msfl_handle* h,
                             const msfl_point* corner, int n_corner,
                             const msfl_point* surf, int n_surf,
                             const double* poses, int n_poses, double max_dist,
                             msfl_pose_score* scores, float* d2_out, int* nn_out, msfl_mem mem);
msfl_status msfl_score_poses_batch(msfl_handle* h, int n_scans,
                                   const msfl_point* corner, const int* corner_off,
                                   const msfl_point* surf, const int* surf_off,
                                   const double* poses, const int* pose_off,
                                   double max_dist, msfl_pose_score* scores, msfl_mem mem);

/* Resident pair maps: the two halves of msfl_match_pairs_batch on their own, and the fitness against the pairs' maps.
   The index over P maps is most of what a pairs call costs (docs/kernels/pairs.md), and a second registration round, a
   yaw lattice per candidate and the fitness of the result all want the same index.

   msfl_set_pair_maps: the index half.  Arguments, limits (at most 65 535 pairs, cell-table and 2^28-point capacity) and
   offset rules (HOST arrays, non-decreasing, need not start at 0) of msfl_match_pairs_batch.  The handle's resident single
   map is replaced, as there.  With MSFL_MEM_DEVICE the call is asynchronous, and the caller's map arrays are not needed
   once the stream has passed it: the index holds its own sorted copy.  n_pairs == 0 changes nothing.
   The pair index stays resident until msfl_set_map, the next msfl_set_pair_maps (also one that fails) or the next
   msfl_match_pairs_batch, which leaves ITS index resident in the same way.

   msfl_score_pairs: msfl_score_poses_batch with scan p scored at the poses [pose_off[p], pose_off[p+1]) against pair map p
   only.  Record, arithmetic, tie rule, fixed-point sums, max_dist rules, non-finite handling and memory kinds are the ones
   described above.  What differs:
     - d2_out / nn_out are allowed, and ragged: the row of a hypothesis of scan p has F(p) = n_corner(p) + n_surf(p)
       values (corner features first), rows in hypothesis order, sum over p of n_poses(p) x F(p) values in all.
     - nn_out holds the position in pair p's OWN map cloud of the feature's kind (what msfl_set_map on that cloud +
       msfl_score_poses returns).
     - MSFL_NO_MAP without a resident pair index; MSFL_BAD_ARG when n_pairs differs from the pairs it holds.  A pair
       whose map side is empty gives zero inliers of that kind, not an error.
   msfl_score_poses(_batch) keeps answering MSFL_NO_MAP while a pair index is resident.

   msfl_match_pairs_resident: the registration half, against the resident pair index: arguments, per-pair
   MSFL_MAP_TOO_SMALL preset and every opt-in feature (uncertainty, prior, degeneracy, rejection) as in
   msfl_match_pairs_batch, whose results msfl_set_pair_maps + this call equal bit for bit.  It does not consume the index
   and may be called any number of times; msfl_score_pairs calls in between change nothing in it.  MSFL_NO_MAP /
   MSFL_BAD_ARG as for msfl_score_pairs. */
msfl_status msfl_set_pair_maps(msfl_handle* h, int n_pairs,
                               const msfl_point* map_corner, const int* map_corner_off,
                               const msfl_point* map_surf, const int* map_surf_off, msfl_mem mem);
msfl_status msfl_score_pairs(msfl_handle* h, int n_pairs,
                             const msfl_point* corner, const int* corner_off,
                             const msfl_point* surf, const int* surf_off,
                             const double* poses, const int* pose_off,
                             double max_dist, msfl_pose_score* scores, float* d2_out, int* nn_out, msfl_mem mem);
msfl_status msfl_match_pairs_resident(msfl_handle* h, int n_pairs,
                                      const msfl_point* corner, const int* corner_off,
                                      const msfl_point* surf, const int* surf_off,
                                      double* poses_io, int* status, msfl_match_info* info, msfl_mem mem);

/* Pose search: where in the resident map is this scan, given only a rough guess?  A lattice of yaw x position hypotheses
   round the guess is scored by a HIT COUNT against a bit-per-voxel occupancy volume of the map, the peaks of the score are
   the candidates, and msfl_relocalize finishes them with the exact score and the matcher.  docs/kernels/search.md has the
   definition in full; in short:
     hypothesis  h = ((a nz + kz') ny + ky') nx + kx', n = 2 half + 1 per axis, k = k' - half;
                 pose(a, k): q = normalised(qz(yaw_min + a yaw_step) * q_guess), t = t_guess + step * k, in double.
     volume      one bit per voxel of pitch `step` and feature kind, over the box msfl_search_geometry reports.  A finite map
                 point inside the box sets the voxel (int)floorf((x - origin.x) * inv_step) (f32, per axis) of its kind's
                 volume; with dilate = 1 every voxel of the box within Chebyshev distance 1 of a set one is set too.
     count       for yaw sample a and feature p, v = voxel of transform_point_f32(pose(a, 0), p).  The feature HITS at
                 (a, k) when v + k lies inside the box and that bit is set in the volume of its kind.  The integer shift IS
                 the definition (it is not the voxel of the point transformed by pose(a, k)).  hits[kind][h] counts the hit
                 features; a non-finite feature or transformed point never hits.
     peaks       order: (hits[0] + hits[1] descending, h ascending).  h is a peak when no OTHER hypothesis within nms_cells
                 (Chebyshev, on k) and nms_yaws (on a; cyclic when yaw_wraps) precedes it.  Windows 0 / 0: every h is a peak.
     candidates  the first `capacity` peaks in that order. */
typedef struct msfl_search_config {
  double step;                 /* lattice AND voxel pitch, metres, > 0 */
  int half[3];                 /* lattice half-extents in cells, >= 0 */
  int n_yaw;                   /* >= 1 */
  double yaw_min, yaw_step;    /* yaw sample a = yaw_min + a * yaw_step, radians */
  int yaw_wraps;               /* 0 / 1: the samples close a full turn (for the peak window only) */
  int dilate;                  /* 0 / 1 */
  double range;                /* features are expected within this distance of the sensor; it sizes the volume */
  int nms_cells, nms_yaws;     /* peak windows, >= 0 */
  long long max_volume_bytes;  /* per kind; a larger volume is MSFL_CAPACITY */
} msfl_search_config;

/* step 0.5, half {6, 6, 0}, 24 yaws from 0 in steps of 2 pi / 24, wraps 1, dilate 1, range 100, windows 1 / 1, 64 MiB. */
void msfl_search_default_config(msfl_search_config* cfg);

typedef struct msfl_search_geom {
  float origin[3];             /* low corner of the box: (float)((floor(t_guess / step) - ext) * step), in double until the cast */
  float inv_step;              /* (float)(1 / step) */
  int dims[3];                 /* 2 ext + 1 voxels per axis, ext = half + ceil(range / step) + dilate + 1 */
  int words_per_row;           /* 64-bit words of one x row: ceil(dims[0] / 64) + 1 (the last one stays zero) */
  int n[3];                    /* lattice positions per axis */
  int n_yaw;
  long long n_hypotheses;      /* H = n_yaw n[2] n[1] n[0] */
  long long volume_bytes;      /* one volume of one kind */
  long long scratch_bytes;     /* device scratch msfl_search_poses needs for n_corner + n_surf features (staging of host arrays aside) */
} msfl_search_geom;

/* The geometry rule, on the host alone (no handle, no GPU): what msfl_search_poses will use for this guess and config.
   MSFL_BAD_ARG: null pointer, non-finite guess, step or range not finite and positive, a negative half or window, n_yaw < 1,
   non-finite yaw_min / yaw_step, dilate / yaw_wraps not 0 / 1, negative counts, max_volume_bytes <= 0.
   MSFL_CAPACITY (out is still filled where it can be): a volume above max_volume_bytes, a dimension above 2^20 voxels,
   more than 2^24 hypotheses, 2^24 features or more of a kind, or more than 2^26 (yaw, feature) table entries. */
msfl_status msfl_search_geometry(const double guess[7], const msfl_search_config* cfg, int n_corner, int n_surf,
                                 msfl_search_geom* out);

typedef struct msfl_pose_candidate {
  double pose[7];              /* pose(a, k) */
  int h;                       /* hypothesis index */
  int a, kx, ky, kz;           /* lattice coordinates, k in [-half, half] */
  int hits[2];                 /* corner, surf */
  int reserved_;
} msfl_pose_candidate;

/* The search itself.
     corner/surf : the scan's features, sensor frame, as in msfl_score_poses.
     candidates  : `capacity` records, 1 <= capacity <= 1024; *n_out of them are written (fewer when there are fewer peaks).
                   In device memory the slots past *n_out are written too, all zero; in host memory they are left alone.
     hits_out    : optional (NULL: not wanted), 2 x H int32: hits[kind][h] over the WHOLE lattice.
   guess and cfg are HOST data in both memory kinds.  With MSFL_MEM_DEVICE corner, surf, candidates, n_out and hits_out are
   device pointers and the call is asynchronous on the handle's stream, ordered after a preceding asynchronous msfl_set_map.
   Refusals, all before anything is staged or launched: MSFL_NO_MAP without a resident single map (also while a pair index is
   resident); MSFL_BAD_ARG / MSFL_CAPACITY as for msfl_search_geometry; MSFL_BAD_ARG for a capacity outside 1 .. 1024.
   An empty map side gives zero hits of that kind.  The call works in scratch of its own and reads the map's point arrays
   only: a matcher or scoring call after it is bit-identical to one without it. */
msfl_status msfl_search_poses(msfl_handle* h,
                              const msfl_point* corner, int n_corner,
                              const msfl_point* surf, int n_surf,
                              const double guess[7], const msfl_search_config* cfg,
                              msfl_pose_candidate* candidates, int capacity, int* n_out, int* hits_out, msfl_mem mem);

typedef struct msfl_reloc_result {
  double pose[7];                  /* the refined pose */
  msfl_pose_candidate candidate;   /* where it started */
  msfl_pose_score coarse;          /* msfl_score_poses at the candidate's pose */
  msfl_pose_score refined;         /* msfl_score_poses at the refined pose */
  int status;                      /* per-scan status of the registration */
  int accepted;                    /* (refined.inliers[0] + refined.inliers[1]) / (n_corner + n_surf) >= min_fitness */
} msfl_reloc_result;

/* Search, verify, refine, verify again: a composition of public calls and no arithmetic of its own.
     1. msfl_search_poses for n_candidates candidates;
     2. msfl_score_poses(max_dist) at their poses; order: exact inliers (both kinds) descending, fixed-point sum (both kinds)
        ascending, candidate order;
     3. msfl_match_scan2map_batch of the first n_refine in that order, each from its candidate pose;
     4. msfl_score_poses(max_dist) at the refined poses; the records leave sorted by rule 2 on the refined scores (ties: step 2's order).
   *n_out = min(n_refine, candidates found) records are written; every byte equals what a caller chaining the four calls gets.
   `mem` says where corner / surf live; guess, cfg, results and n_out are host data and the call returns when it is done.
   MSFL_BAD_ARG besides the rules of the four calls: n_candidates outside 1 .. 1024, n_refine outside 1 .. n_candidates,
   capacity < n_refine, a NaN min_fitness.  Towards the handle's state (record sinks, pose priors, timing, the poses and
   records a matcher call leaves behind) the call counts as ONE msfl_match_scan2map_batch call of *n_out registrations. */
msfl_status msfl_relocalize(msfl_handle* h,
                            const msfl_point* corner, int n_corner,
                            const msfl_point* surf, int n_surf,
                            const double guess[7], const msfl_search_config* cfg, int n_candidates,
                            double max_dist, int n_refine, double min_fitness,
                            msfl_reloc_result* results, int capacity, int* n_out, msfl_mem mem);

/* The search against the resident PAIR index (msfl_set_pair_maps / msfl_match_pairs_batch): scan p round guess p against pair
   map p, all n_pairs searches in one chain of launches.  No new arithmetic: for every pair p the candidates (row p of
   `candidates`), n_out[p], the counts and, in device memory, the all-zero slots past n_out[p] are byte for byte what
   msfl_set_map(pair p's corner map, pair p's surf map) followed by msfl_search_poses(scan p, guesses + 7 p, cfg, ..., capacity,
   ...) writes.  The geometry of pair p is msfl_search_geometry(guesses + 7 p, cfg, n_corner(p), n_surf(p)); with the one shared
   cfg only `origin` differs between pairs, and the yaw lattice of pair p is round guess p's quaternion.
     corner/surf, corner_off/surf_off : the concatenated scans and their n_pairs + 1 prefix offsets (HOST arrays), by the
                   offset rules of msfl_score_pairs.
     guesses     : 7 x n_pairs doubles; guesses and cfg are HOST data in both memory kinds.
     candidates  : n_pairs x capacity records, row p = pair p; 1 <= capacity <= 1024.  n_out: n_pairs counts.
     hits_out    : optional, n_pairs x 2 x H int32, [p][kind][h].
   With MSFL_MEM_DEVICE corner, surf, candidates, n_out and hits_out are device pointers, and the call is asynchronous on the
   handle's stream, ordered after an asynchronous msfl_set_pair_maps; it never waits for the device.  With host memory the
   slots past n_out[p] are left alone.
   Refusals, all before anything is staged or launched, in this order: MSFL_BAD_ARG for an unknown memory kind, negative
   counts, null pointers, bad offsets or a capacity outside 1 .. 1024; what msfl_search_geometry answers for the first pair it
   refuses (msfl_last_error names the pair); MSFL_NO_MAP without a resident pair index (also while a single map is resident),
   MSFL_BAD_ARG when n_pairs is not the number of pairs it holds.  msfl_search_poses and msfl_relocalize keep answering
   MSFL_NO_MAP while a pair index is resident.  A pair with an empty map side or no features of a kind has zero hits of that
   kind.  n_pairs == 0 is refused or accepted as by msfl_score_pairs.
   The pairs are processed in chunks that fit a fixed scratch budget (MSFL_SEARCH_CHUNK_PAIRS in the environment forces the
   chunk size); the results do not depend on the chunking.  The call works in the search scratch only and reads the pair
   index's point arrays and cell tables: msfl_match_pairs_resident and msfl_score_pairs after it are bit-identical to the same
   calls without it.  Not provided: a msfl_relocalize over pairs (examples/close_loop.py chains the calls), and a batched
   search of many scans against the single map. */
msfl_status msfl_search_pairs(msfl_handle* h, int n_pairs,
                              const msfl_point* corner, const int* corner_off,
                              const msfl_point* surf, const int* surf_off,
                              const double* guesses, const msfl_search_config* cfg,
                              msfl_pose_candidate* candidates, int capacity, int* n_out, int* hits_out, msfl_mem mem);

/* Kernel-level entry points (the two halves of one outer iteration), exposed so that parity tests
   can pin the data association and the solver separately:
     msfl_associate_scan2map : mapping_scan_matcher.cc:109-246 at a fixed pose.  records_out gets
                               (n_corner + n_surf) x 6 doubles {C[3], N[3]} in feature order (corner
                               first); a rejected feature is all zeros.  For an edge C = point_a and
                               N = (a-b).normalized() (:150-158); for a plane C = center, N = norm (:238).
     msfl_solve_records      : one ceres::Solve (:250-259) on caller-provided records.
   Host pointers only. */
msfl_status msfl_associate_scan2map(msfl_handle* h,
                                    const msfl_point* corner, int n_corner,
                                    const msfl_point* surf, int n_surf,
                                    const double pose[7], double* records_out);
msfl_status msfl_solve_records(msfl_handle* h,
                               const msfl_point* corner, int n_corner,
                               const msfl_point* surf, int n_surf,
                               const double* records, double pose_io[7], msfl_match_info* info);

/* Optional IMU-deskew inputs for the is_initialized branch (mapping_scan_matcher.cc:84-94,
   119-121,154-166,189-191,224-236).  The per-point (delta_q, delta_p) = GetDeltaQP(preintegration,
   dt) (scan_undistortion.cc:22-42) are computed by the caller (IMU pre-integration is outside the
   hot path); the velocity block is held constant by the reference (.cc:94), so only the pose is
   optimised.  Layout: delta_q as [qx qy qz qw], one per corner then one per surf feature. */
typedef struct msfl_deskew {
  const double* corner_dq;  /* n_corner x 4 */
  const double* corner_dp;  /* n_corner x 3 */
  const double* surf_dq;    /* n_surf x 4 */
  const double* surf_dp;    /* n_surf x 3 */
  double velocity[3];       /* bias_j.head<3>() (Vi, .cc:107) */
  double gravity[3];        /* gravity_vector */
} msfl_deskew;

/* As msfl_match_scan2map with the Deskew factors (lidar_factor.cc:46-100).  Host pointers only. */
msfl_status msfl_match_scan2map_deskew(msfl_handle* h,
                                       const msfl_point* corner, int n_corner,
                                       const msfl_point* surf, int n_surf,
                                       const msfl_deskew* deskew,
                                       double pose_io[7], msfl_match_info* info);

/* Kernel-level entry points of the deskew branch (the two halves of one outer iteration of msfl_match_scan2map_deskew),
   exposed like msfl_associate_scan2map / msfl_solve_records so that parity tests can pin them separately:
     msfl_associate_scan2map_deskew : one association pass at a fixed pose through the launch pair the deskew matcher takes
                                      (the counting 5-NN instantiation after msfl_set_timing(h, 3)).  Feature i is searched at
                                      pose * {q^-1 (V dt_i - G dt_i^2 / 2) + dp_i, dq_i} (:120 / :190).  records_out gets
                                      (n_corner + n_surf) x 6 doubles {C', N} in feature order (corner first), with
                                      C' = C - (V dt_i - G dt_i^2 / 2); a rejected feature is all zeros.  points_out gets
                                      (n_corner + n_surf) x 3 doubles p'_i = dq_i p_i + dp_i, whether accepted or not.
     msfl_solve_records_deskew      : msfl_solve_records with the residual points given as f64 `points`
                                      ((n_corner + n_surf) x 3, corner rows first, non-null even for an empty problem): the
                                      solve, rejection and uncertainty kernels run their deskew branch (no plane cache, points
                                      from global memory).  MSFL_SOLVE_RECORDS_BLOCK and every registration option apply as for
                                      msfl_solve_records.  The clouds give the counts only; their xyz are not read by the solve.
   Host pointers only. */
msfl_status msfl_associate_scan2map_deskew(msfl_handle* h,
                                           const msfl_point* corner, int n_corner,
                                           const msfl_point* surf, int n_surf,
                                           const msfl_deskew* deskew, const double pose[7],
                                           double* records_out, double* points_out);
msfl_status msfl_solve_records_deskew(msfl_handle* h,
                                      const msfl_point* corner, int n_corner,
                                      const msfl_point* surf, int n_surf,
                                      const double* records, const double* points,
                                      double pose_io[7], msfl_match_info* info);

/* The deskew branch for a batch.  The four per-feature arrays are indexed exactly like the feature arrays
   (corner feature corner_off[b] + k of scan b uses corner_dq[4 * (corner_off[b] + k)] ...), velocity holds
   one Vi per scan; all follow `mem`. */
typedef struct msfl_deskew_batch {
  const double* corner_dq;  /* (corner_off[n_scans]) x 4 */
  const double* corner_dp;  /* ... x 3 */
  const double* surf_dq;
  const double* surf_dp;
  const double* velocity;   /* n_scans x 3 */
  double gravity[3];
} msfl_deskew_batch;

msfl_status msfl_match_scan2map_deskew_batch(msfl_handle* h, int n_scans,
                                             const msfl_point* corner, const int* corner_off,
                                             const msfl_point* surf, const int* surf_off,
                                             const msfl_deskew_batch* deskew,
                                             double* poses_io, int* status, msfl_match_info* info, msfl_mem mem);

/* ------------------------------------------------------------------------------------------ */
/* stage B — scan-to-scan registration                                                        */
/*   replaces OdometryScanMatcher::MatchScan2Scan (odometry_scan_matcher.h:10-12, .cc:43-285)  */
/* ------------------------------------------------------------------------------------------ */

/* A ring-ordered feature cloud of PointXYZIRT (common.h:44-62): points + ring ids. */
typedef struct msfl_ring_cloud {
  const msfl_point* pts;
  const uint16_t*   ring;
  int               n;
} msfl_ring_cloud;

/*   last_less_sharp / last_less_flat : scan_last.cloud_corner_less_sharp / cloud_surf_less_flat
     curr_sharp / curr_flat           : scan_curr.cloud_corner_sharp / cloud_surf_flat
     pose_io                          : pose_estimate_curr2last, in/out.
   Returns MSFL_TOO_FEW_CORRESPONDENCES where the reference returns false (.cc:262-267); the
   pose then holds the result of the outer iterations completed so far. */
msfl_status msfl_match_scan2scan(msfl_handle* h,
                                 const msfl_ring_cloud* last_less_sharp,
                                 const msfl_ring_cloud* last_less_flat,
                                 const msfl_ring_cloud* curr_sharp,
                                 const msfl_ring_cloud* curr_flat,
                                 double pose_io[7], msfl_match_info* info,
                                 msfl_mem mem);

/* B independent (last, curr) pairs.  Each of the four feature sets is concatenated over the
   batch with B+1 prefix offsets. */
typedef struct msfl_ring_cloud_batch {
  const msfl_point* pts;
  const uint16_t*   ring;
  const int*        off;   /* n_scans + 1 */
} msfl_ring_cloud_batch;

msfl_status msfl_match_scan2scan_batch(msfl_handle* h, int n_scans,
                                       const msfl_ring_cloud_batch* last_less_sharp,
                                       const msfl_ring_cloud_batch* last_less_flat,
                                       const msfl_ring_cloud_batch* curr_sharp,
                                       const msfl_ring_cloud_batch* curr_flat,
                                       double* poses_io, int* status, msfl_match_info* info,
                                       msfl_mem mem);

/* ------------------------------------------------------------------------------------------ */
/* stage A — feature extraction                                                               */
/*   replaces RealHandleLaserCloudMessage (msf_loam_node.cc:160-378) between pcl::fromROSMsg   */
/*   (:166-167) and LaserOdometry::AddLaserScan (:373).                                        */
/* ------------------------------------------------------------------------------------------ */

/* Output of one extraction = the five clouds of TimestampedPointCloud<PointXYZIRT>
   (timestamped_pointcloud.h:11-42).  cloud_full_res is the ring-concatenated valid cloud
   (msf_loam_node.cc:188-195) with t = relative time; the four feature clouds are returned as
   INDEX LISTS into cloud_full_res (the reference push_back()s copies of those same points), in
   the reference's push order.  Caller allocates: full_pts/full_ring/curvature/label with capacity
   n_in, the four index arrays with capacity n_in each.  `extrinsic` (lidar->imu, :367-371) may be
   NULL = identity (the shipped config, config/lio-sam-config2.json:7-20). */
typedef struct msfl_features {
  msfl_point* full_pts;    /* out: n_full points */
  uint16_t*   full_ring;   /* out */
  float*      curvature;   /* out: cloud_curvatures (valid for i in [5, n_full-5)) */
  uint8_t*    label;       /* out: PointLabel 0 UNKNOWN 1 SHARP 2 LESS_SHARP 3 FLAT (:68-77) */
  int*        sharp_idx;       /* out */
  int*        less_sharp_idx;  /* out */
  int*        flat_idx;        /* out */
  int*        less_flat_idx;   /* out */
  int n_full, n_sharp, n_less_sharp, n_flat, n_less_flat;  /* out counts */
} msfl_features;

/*   pts/ring : the sensor cloud as pcl::fromROSMsg delivers it (driver order), n points.
   Returns MSFL_BAD_RING for ring >= 128 (CHECK at :136), MSFL_BAD_ARG for an empty valid
   cloud (CHECK at :186,200) and MSFL_CAPACITY for a ring of more than 8128 valid points (the
   per-ring pick state is held on chip; a 128-beam sensor at 2048 columns has 2048 per ring). */
msfl_status msfl_extract_features(msfl_handle* h,
                                  const msfl_point* pts, const uint16_t* ring, int n,
                                  const double* extrinsic_pose7,
                                  msfl_features* out, msfl_mem mem);

/* B scans in one call; scan b owns [off[b], off[b+1]) of pts/ring and writes its outputs at the
   same offsets of the out arrays (index lists are scan-local); counts go to the five
   n_* arrays of length B. */
typedef struct msfl_features_batch {
  msfl_point* full_pts;  uint16_t* full_ring;  float* curvature;  uint8_t* label;
  int* sharp_idx;  int* less_sharp_idx;  int* flat_idx;  int* less_flat_idx;
  int* n_full;  int* n_sharp;  int* n_less_sharp;  int* n_flat;  int* n_less_flat;  /* B each */
} msfl_features_batch;

msfl_status msfl_extract_features_batch(msfl_handle* h, int n_scans,
                                        const msfl_point* pts, const uint16_t* ring,
                                        const int* off,
                                        msfl_features_batch* out, int* status, msfl_mem mem);

/* ------------------------------------------------------------------------------------------ */
/* helpers on the caller side of the path: pcl::VoxelGrid down-sampling of  */
/* the scan features before MatchScan2Map (laser_mapping.cc:264-270) and TransformPointCloud.  */
/* ------------------------------------------------------------------------------------------ */

/* Centroid voxel filter with PCL VoxelGrid semantics (leaf cube, centroid of x,y,z,t per
   occupied voxel, output ordered by voxel index).  out has capacity n; *n_out receives the
   count.  Non-finite points are DROPPED, as pcl::VoxelGrid::applyFilter does for a cloud that is
   not dense (`if (!input_->is_dense) if (!pcl_isfinite(...)) continue;`): a stable device-side
   compaction followed by the same filter.  (For a cloud flagged dense PCL does not look and its
   result is undefined; the reference's clouds never hold such a point, msf_loam_node.cc:85-111.)
   The batch forms below REFUSE a cloud with a non-finite point (MSFL_BAD_ARG): their inputs are
   the extraction's own outputs.
   MSFL_CAPACITY, *n_out = 0: the leaf is too small for the cloud's extent -- its bounding box holds
   more than 2^31 - 1 voxels, or a voxel coordinate floor(p / leaf) reaches 1e9 in magnitude
   (pcl::VoxelGrid warns "leaf size is too small" and does not filter such a cloud). */
msfl_status msfl_voxel_downsample(msfl_handle* h,
                                  const msfl_point* pts, int n, float leaf,
                                  msfl_point* out, int* n_out, msfl_mem mem);

/* The same filter over n_clouds clouds in one pass (the device-resident batch pipeline between
   msfl_extract_features_batch and msfl_match_scan2map_batch).  Cloud b occupies the region
   [off[b], off[b+1]) of `pts`; with `idx` it is the points pts[off[b] + idx[off[b] + k]],
   k < count[b] — exactly how msfl_features_batch lays out its index lists and counts, so a feature
   list is filtered straight out of the extraction's output.  idx == NULL: the region itself;
   count == NULL: the whole region.  `off` is a host array (like every batch call), pts / idx /
   count / out follow `mem`.  The filtered clouds are written back to back into `out` (capacity
   off[n]-off[0] points) and out_off (HOST, n_clouds+1) receives their boundaries; the call
   synchronises once to deliver them.  A cloud holding a non-finite point makes the call return
   MSFL_BAD_ARG (the clouds before it are still delivered).  A cloud whose leaf is too small for
   its extent (see msfl_voxel_downsample) makes the call return MSFL_CAPACITY: that cloud's output
   range is empty (out_off[b] == out_off[b+1]) and every other cloud of the batch is delivered.
   msfl_voxel_downsample_batch_pair reports it the same way, per list: the other list is unaffected. */
msfl_status msfl_voxel_downsample_batch(msfl_handle* h, int n_clouds,
                                        const msfl_point* pts, const int* idx, const int* off,
                                        const int* count, float leaf,
                                        msfl_point* out, int* out_off, msfl_mem mem);

/* Two index lists over the same clouds in one call: the corner (0.2 m) and surf (0.4 m) filters that
   the mapping thread runs back to back on every scan (laser_mapping.cc:264-270).  Same results as two
   msfl_voxel_downsample_batch calls (list a, then list b; every argument as there, idx_* and count_*
   required); with device memory both filters are enqueued before the one synchronisation that
   delivers both boundary tables, so the small corner kernels do not wait for a host round trip. */
msfl_status msfl_voxel_downsample_batch_pair(msfl_handle* h, int n_clouds,
                                             const msfl_point* pts, const int* off,
                                             const int* idx_a, const int* count_a, float leaf_a,
                                             msfl_point* out_a, int* out_off_a,
                                             const int* idx_b, const int* count_b, float leaf_b,
                                             msfl_point* out_b, int* out_off_b, msfl_mem mem);

/* TransformPointCloud (laser_mapping.cc:24-31 -> TransformPoint, rigid_transform.h:131-137): every
   point goes f32 -> f64 -> q*p + t -> f32, t (relative time) is carried over.  pose7 is always a
   host array; in == out is allowed. */
msfl_status msfl_transform_cloud(msfl_handle* h,
                                 const msfl_point* in, int n, const double pose7[7],
                                 msfl_point* out, msfl_mem mem);

/* ------------------------------------------------------------------------------------------ */
/* next row N3: per-point IMU deskew.                                          */
/* ------------------------------------------------------------------------------------------ */

/* What GetDeltaQP reads of an IntegrationBase (integration_base.h:62-66): per IMU sample the
   cumulative time and the pre-integrated rotation / position.  Always host arrays (a scan spans
   ~40-50 samples); n >= 2, sum_dt non-decreasing. */
typedef struct msfl_preintegration {
  const double* sum_dt;   /* n */
  const double* delta_q;  /* n x 4, [qx qy qz qw] */
  const double* delta_p;  /* n x 3 */
  int n;
} msfl_preintegration;

/* GetDeltaQP (scan_undistortion.cc:22-42) for every point's relative time pts[i].t: upper_bound
   over sum_dt, Eigen slerp of delta_q (no normalisation), lerp of delta_p.  Writes the arrays
   msfl_deskew takes (dq n x 4 [x y z w], dp n x 3).  Returns MSFL_BAD_ARG where the reference
   CHECK-aborts (a time outside [sum_dt.front(), sum_dt.back()], :26-30).  A time equal to
   sum_dt.back() makes the reference index one past the end (:37-39); here it yields the last
   sample (s = 1). */
msfl_status msfl_delta_qp(msfl_handle* h, const msfl_preintegration* pre,
                          const msfl_point* pts, int n, double* dq, double* dp, msfl_mem mem);

/* The deskew pass of LaserMapping (laser_mapping.cc:197-211), in place on one cloud:
     p <- (dq(t) * p + R_odom^-1 * (velocity * t - 0.5 * gravity * t * t) + dp(t)).cast<float>()
   rot_odom_xyzw = pose_odom_scan2world_.rotation() as [qx qy qz qw]. */
/* Both in-place passes are all-or-nothing: when any time stamp is refused (MSFL_BAD_ARG) the cloud, host or device, is
   left exactly as it was. */
msfl_status msfl_deskew_cloud(msfl_handle* h, const msfl_preintegration* pre,
                              msfl_point* pts_io, int n, const double rot_odom_xyzw[4],
                              const double velocity[3], const double gravity[3], msfl_mem mem);

/* UndistortScanInternal (scan_undistortion.cc:5-19), in place: p <- dq(t).cast<float>() * p.
   MSFL_BAD_ARG also for a negative time (CHECK_GE, :12). */
msfl_status msfl_undistort_cloud(msfl_handle* h, const msfl_preintegration* pre,
                                 msfl_point* pts_io, int n, msfl_mem mem);

/* ------------------------------------------------------------------------------------------ */
/* next row N1: the local map store kept resident on the device.               */
/*   replaces HybridGrid (src/slam/map/hybrid_grid.h:27-39, hybrid_grid.cc:462-534), owned by   */
/*   LaserMapping as hybrid_grid_map_corner_ / hybrid_grid_map_surf_ (laser_mapping.h:77-78).   */
/* ------------------------------------------------------------------------------------------ */

typedef struct msfl_grid_s msfl_grid;

/* HybridGrid(resolution) (laser_mapping.cc:44-45: 3.0 m cells) plus the leaf of the pcl::VoxelGrid its
   owner passes to InsertScan (laser_mapping.cc:60-68: 0.2 corner / 0.4 surf).  The grid works on
   `h`'s stream and must be destroyed before `h`. */
msfl_status msfl_grid_create(msfl_handle* h, float resolution, float leaf, msfl_grid** out);
void msfl_grid_destroy(msfl_grid* g);

/* HybridGrid::InsertScan (hybrid_grid.cc:503-521): append every point to the cell
   lround(p / resolution) and VoxelGrid-filter the touched cells in place.  `pts` are in the map
   frame (the caller transforms them, laser_mapping.cc:330-338).  MSFL_CAPACITY if a point leaves
   the +-8192-cell range of the reference (the map is then left unchanged). */
msfl_status msfl_grid_insert_scan(msfl_grid* g, const msfl_point* pts, int n, msfl_mem mem);

/* HybridGrid::GetSurroundedCloud (hybrid_grid.cc:470-501): union of the cells hit by
   pose_f32 * p + (i,j,k) m, (i,j,k) in {-1,0,1}^3, over the scan points with |p| <= 60 m.
   `scan` is in the scan frame, pose7 maps scan -> map.  Cells come out in ascending (iz,iy,ix)
   order (the reference iterates an unordered set: unspecified).  *n_out receives the full count;
   MSFL_CAPACITY if it exceeds `capacity` (the first `capacity` points are still written).
   With MSFL_MEM_DEVICE the result can be handed straight to msfl_set_map. */
msfl_status msfl_grid_get_surrounded(msfl_grid* g, const msfl_point* scan, int n, const double pose7[7],
                                     msfl_point* out, int capacity, int* n_out, msfl_mem mem);

msfl_status msfl_grid_size(msfl_grid* g, int* n_points, int* n_cells);
/* all points, cells ascending (the reference dumps the map to PLY on shutdown, laser_mapping.cc:95-113) */
msfl_status msfl_grid_dump(msfl_grid* g, msfl_point* out, int capacity, int* n_out, msfl_mem mem);

/* {ix, iy, iz, count} of every cell into the host array `cells` (capacity x 4 ints), in the order of msfl_grid_dump: the dump's
   points [sum of the counts before, + count) belong to that cell.  A dump alone cannot be split back into cells (a centroid may
   round across the boundary of the cell that owns it); with this list a saved map can be read again cell by cell.  *n_out receives
   the number of cells; MSFL_CAPACITY if it exceeds `capacity` (the first `capacity` cells are still written). */
msfl_status msfl_grid_dump_cells(msfl_grid* g, int* cells, int capacity, int* n_out);

/* {n_points, n_cells, pool_top, pool_capacity_points, cell_capacity, device_bytes}: live sizes, the first free slot of the point
   pool, the capacities of the pool and of the cell table, and the device memory the store holds.  Synchronises like msfl_grid_size. */
msfl_status msfl_grid_stats(msfl_grid* g, long long out[6]);

/* Windowed local map.  HybridGrid never removes a cell, so a store that is only inserted into grows with the distance driven.
   msfl_grid_crop forgets every cell outside a window of cells: with c = lround(f32(center) / resolution) per axis (the cell
   InsertScan files a point at `center` under), cell (ix, iy, iz) is kept iff |ix - cx| <= half_cells[0] && |iy - cy| <=
   half_cells[1] && |iz - cz| <= half_cells[2].  Kept cells are untouched (points, order, what the surround query delivers); the
   room of the others is reclaimed by the store's next compaction.  GetSurroundedCloud reads nothing beyond 60 m + 1 m of the
   sensor (hybrid_grid.cc:474-485), so a window of 23 cells of 3 m around the sensor takes nothing from the registration of a scan
   taken there.  What it does take away are returns from beyond the window, which the unbounded map would have kept until the
   sensor came within 60 m of them: with a sensor whose range stays inside the window nothing changes at all.
     evicted == NULL : the evicted points are dropped.
     otherwise       : `evicted` (`capacity` points; host or device memory as `mem` says) receives them, cells ascending and in
                       stored order inside a cell: the order msfl_grid_dump would have delivered them in.  If they are more than
                       `capacity` the crop is refused as a whole: the map is unchanged, info->applied = 0, the counts in `info`
                       say how much room is needed, MSFL_CAPACITY is returned.
   Evicted points that are inserted again with msfl_grid_insert_scan pass through the voxel filter again (they are centroids
   already) and are filed by their own coordinates; msfl_grid_crop_tiles + msfl_grid_load_cells below bring a tile back as it was.
   MSFL_BAD_ARG: a negative half_cells entry, a centre that is not finite (in f32), info == NULL. */
typedef struct msfl_grid_crop_info {
  int n_cells_evicted, n_points_evicted;   /* what this crop removed (full counts, also when it was refused) */
  int n_cells, n_points;                   /* live sizes after the crop */
  int center_cell[3];                      /* (ix, iy, iz) the window was centred on */
  int applied;                             /* 1, or 0 when the crop was refused: map unchanged */
} msfl_grid_crop_info;

msfl_status msfl_grid_crop(msfl_grid* g, const double center[3], const int half_cells[3],
                           msfl_point* evicted, int capacity, msfl_mem mem, msfl_grid_crop_info* info);

/* msfl_grid_crop with `evicted` required, which also says WHICH cells went: `evicted_cells` (host, cell_capacity x 4 ints) receives
   {ix, iy, iz, count} of the evicted cells in the order of `evicted` (cells ascending).  The pair goes unchanged into
   msfl_grid_load_cells.  More evicted cells than `cell_capacity` refuses the crop as a whole exactly as too many points does
   (map unchanged, info->applied = 0, the counts in `info` say how much room is needed, MSFL_CAPACITY).
   MSFL_BAD_ARG: as msfl_grid_crop; evicted == NULL, evicted_cells == NULL, a negative capacity. */
msfl_status msfl_grid_crop_tiles(msfl_grid* g, const double center[3], const int half_cells[3], msfl_point* evicted, int capacity,
                                 int* evicted_cells, int cell_capacity, msfl_mem mem, msfl_grid_crop_info* info);

/* Load dumped or evicted cells back, bit for bit.
     cells : host array of n_cells x 4 ints {ix, iy, iz, count}: what msfl_grid_dump_cells / msfl_grid_crop_tiles write.
     pts   : n_points points (host or device memory as `mem` says), the cells' points back to back in list order and, inside a cell,
             in stored order: what msfl_grid_dump and the `evicted` buffer of a crop deliver.
     conflict : optional, host, n_cells ints: 1 where the listed cell is live in the store already, else 0.
   Every listed cell becomes a live cell whose slab is the given points in the given order, untouched: no voxel filter, and the
   cell is NOT re-derived from the coordinates.  The points are trusted to belong to their cell; a dump cannot be checked by
   coordinates, because a stored centroid may round across the boundary of the cell or voxel that owns it.  The new cells' surround
   stamp is 0.  Live cells are untouched: points, order, stamps and what the surround query delivers.  A loaded cell is
   indistinguishable from one that never left, for the surround query and for every later insert that touches it.
   Refused before anything is staged, MSFL_BAD_ARG (msfl_last_error names the rule): info == NULL; cells or pts NULL where needed; a
   negative size; a count <= 0; an index outside [-8192, 8191]; keys not strictly ascending in (iz, iy, ix); counts that do not sum
   to n_points.  n_cells == 0 is a no-op that fills `info` with applied = 1.
   Refused on the device, as a whole (the map is unchanged bit for bit, info->applied = 0, the counts in `info` are filled):
     a listed cell that is live already : MSFL_BAD_ARG; n_conflicts and conflict[] say which.  Load the others with this call and
                                          merge those with msfl_grid_insert_scan, the only way to merge into a live cell.
     a point that is not finite         : MSFL_CAPACITY, the status msfl_grid_insert_scan gives for it. */
typedef struct msfl_grid_load_info {
  int n_cells_loaded, n_points_loaded;   /* what this call added; 0, 0 when it was refused */
  int n_cells, n_points;                 /* live sizes after the call */
  int n_conflicts;                       /* cells of the list that are live in the store already */
  int n_bad_points;                      /* points the insert's key kernel would drop a scan for (not finite) */
  int applied;                           /* 1, or 0: refused as a whole, map unchanged */
  int reserved_;
} msfl_grid_load_info;

msfl_status msfl_grid_load_cells(msfl_grid* g, const int* cells, int n_cells, const msfl_point* pts, int n_points, msfl_mem mem,
                                 int* conflict, msfl_grid_load_info* info);

/* Carve: remove the points a later scan sees through (docs/kernels/grid_store.md, "Carve", has the definition in full).
   HybridGrid never removes a point, so whatever stood somewhere once (a parked car, a person, a closed door) stays in a resident
   map for good.  msfl_grid_carve takes one scan in the sensor frame and the sensor's map pose: a stored point that lies on a ray
   along which the scan measured a return well beyond it is not there any more and leaves the store.
     range image : n_row x n_col pixels over the elevations [elev_low_deg, elev_high_deg) and the full turn; a point's pixel is found by
                   bisection over f32 compares against the host-built tables below (no atan2).  near[pixel] = minimum range r of the
                   scan's points there, +inf when empty.  A point has no pixel when it is not finite, lies on the sensor's axis
                   (x*x + y*y == 0), outside the elevations, or !(r >= min_range) || r > max_range.
     limit image : lim[pixel] = 0 where near[pixel] is empty (no evidence), else the minimum of near over rows +-window_row (clamped
                   to the image) and columns +-window_col (wrapping round the turn).
     the test    : a stored point p goes through the inverse of pose7 exactly as msfl_transform_cloud transforms; it is removed iff
                   it has a pixel and (r * (1 + margin_rel)) + margin_abs < lim[pixel], all in f32.
     the store   : a cell keeps its surviving points in stored order; a cell left with none leaves the table; every other cell, the
                   surround stamps and the order of the table stay as they are.  The pool is not compacted.
     removed     : NULL, or `capacity` points (host or device memory as `mem` says) that receive the removed points in the order of
                   msfl_grid_dump (cells ascending, stored order inside a cell).  More of them than `capacity` refuses the call as a
                   whole exactly like msfl_grid_crop: map unchanged bit for bit, info->applied = 0, the counts are filled, MSFL_CAPACITY.
     scan, pose7 : host or device memory as `mem` says.  n == 0 is a scan that saw nothing: nothing is removed.
     cfg         : NULL = msfl_carve_default_config.
   MSFL_BAD_ARG: info or pose7 NULL, n < 0, scan NULL with n > 0, removed with a negative capacity, a configuration outside
   n_col even in [2, 2048], n_row in [1, 128], -90 < elev_low_deg < elev_high_deg < 90, 0 <= min_range < max_range, margins >= 0,
   windows in [0, 4], everything finite; a pose that is not finite (a device-resident one is refused on the device: map unchanged,
   info->applied = 0, the same status). */
typedef struct msfl_carve_config {
  int n_col, n_row;                        /* columns of the full turn (even), rows between the two elevations */
  float elev_low_deg, elev_high_deg;       /* row k spans the elevations [e_k, e_k+1), e_k = low + (high - low) k / n_row */
  float min_range, max_range;              /* metres; scan points and stored points outside have no pixel */
  float margin_abs, margin_rel;            /* how far beyond a stored point the scan must have seen */
  int window_col, window_row;              /* half widths of the limit image's window */
} msfl_carve_config;

/* The 16-beam sensor of the synthetic worlds (-15 .. +15 degrees, 2 degrees apart): 720 x 16 pixels, one beam per row and the rows
   centred on the beams (-16 .. +16 degrees), 0.3 .. 100 m, margins 0.3 m + 2 %, a window of 1 x 1 pixels. */
void msfl_carve_default_config(msfl_carve_config* cfg);

/* The tables the kernels bisect over, built in double and rounded to f32 (pure host function, no handle):
     cc[k], cs[k] = cos, sin(2 pi k / n_col), k < n_col / 2;   ec[k], es[k] = cos, sin(e_k in radians), k <= n_row.
   cc, cs: n_col / 2 floats each; ec, es: n_row + 1 floats each.  MSFL_BAD_ARG: a null pointer, a configuration outside the limits. */
msfl_status msfl_carve_tables(const msfl_carve_config* cfg, float* cc, float* cs, float* ec, float* es);

typedef struct msfl_grid_carve_info {
  int n_points_removed, n_cells_emptied;   /* what this call removed (full counts, also when it was refused) */
  int n_cells, n_points;                   /* live sizes after the call */
  int n_tested;                            /* stored points that had a pixel */
  int n_pixels;                            /* non-empty pixels of the scan's range image */
  int applied;                             /* 1, or 0 when the call was refused: map unchanged */
  int reserved_;
} msfl_grid_carve_info;

msfl_status msfl_grid_carve(msfl_grid* g, const msfl_point* scan, int n, const double pose7[7], const msfl_carve_config* cfg,
                            msfl_point* removed, int capacity, msfl_mem mem, msfl_grid_carve_info* info);

/* Render and scan novelty: the carve's mirror image (docs/kernels/novelty.md has the definition in full).  The carve asks which
   STORED points a scan sees through; these calls ask which SCAN points stand in space the map saw through.
     msfl_grid_render   the range image the store predicts for a sensor at pose7: every stored point goes through the inverse of pose7
                        exactly as the carve's test takes it (the pose inverted in f64, the point f32 -> f64 -> q' p + t' -> f32, the
                        quaternion as given), then through the carve's pixel rule; range_img[row * n_col + col] is the minimum range of
                        the points with that pixel, +inf (bits 0x7f800000) where there is none.  accumulate = 0 sets the image to +inf
                        first; accumulate = 1 takes the minimum into the image that is there, so the corner store and then the surf store
                        give one image.  The minimum is an unsigned one on the bit patterns: the order of the calls does not matter.
                        Only n_col, n_row, the elevations and the ranges of cfg matter here.  The store is only read.
     msfl_scan_novelty  one class per scan point (sensor frame) against such an image.  For the point's pixel (row, col) the window
                        covers the rows row +- window_row clamped to the image (a repeated edge row is counted again) and the columns
                        col +- window_col wrapping round the turn; support = the window positions whose map pixel is not +inf, mlim =
                        the unsigned minimum of the map pixels over the window.  An empty centre pixel does not void the window.
                          MSFL_NOV_NONE      the point has no pixel
                          MSFL_NOV_UNSEEN    support < min_support: the map holds no evidence round this ray
                          MSFL_NOV_IN_FRONT  otherwise, and (r * (1 + margin_rel)) + margin_abs < mlim in f32: everything the map holds
                                             round this ray lies well beyond the return
                          MSFL_NOV_COVERED   otherwise
                        IN_FRONT means new relative to the map, not moving: a newly placed static object is labelled the same way.
     masked_out  : NULL, or one point per point: scan[i] when keep_classes has bit (1 << class), else x = y = z = NaN and the fourth
                   field untouched (the contract of msfl_segment_scans: it goes straight into msfl_extract_features* or
                   msfl_slam_add_scan).  Must not overlap scan.
     mem         : where pose7, range_img / map_img, scan and the outputs live.  Configurations and info records are HOST data.
     info        : NULL with device memory: the call only enqueues on the handle's stream and never waits.  Non-NULL: the counts are read
                   back (the call synchronises).  A host-memory call always waits.
     cfg         : NULL = msfl_carve_default_config / msfl_novelty_default_config.
   MSFL_BAD_ARG, before anything is staged or launched: a null g / h / pose7 / range_img / map_img, n < 0, scan or cls_out NULL with
   n > 0, masked_out overlapping scan, a configuration outside the limits of msfl_carve_config, min_support outside
   [1, (2 window_col + 1)(2 window_row + 1)], keep_classes outside [0, 15], a host pose that is not finite.  A device-resident pose
   that is not finite is refused on the device: nothing is rendered (the image is all +inf with accumulate = 0 and untouched with
   accumulate = 1), info->applied = 0 and the status is MSFL_BAD_ARG when info is read back.  Image values that are neither positive
   floats nor +inf are the caller's error: they are compared by bit pattern and no index depends on them. */
typedef struct msfl_grid_render_info {
  int n_tested;                            /* stored points that had a pixel */
  int applied;                             /* 1, or 0 when a device-resident pose was refused: nothing rendered */
} msfl_grid_render_info;

msfl_status msfl_grid_render(msfl_grid* g, const double pose7[7], const msfl_carve_config* cfg, float* range_img, int accumulate,
                             msfl_mem mem, msfl_grid_render_info* info);

enum { MSFL_NOV_NONE = 0, MSFL_NOV_UNSEEN = 1, MSFL_NOV_COVERED = 2, MSFL_NOV_IN_FRONT = 3, MSFL_NOV_CLASSES = 4 };

typedef struct msfl_novelty_config {
  msfl_carve_config image;                 /* the image geometry, the two margins and the window */
  int min_support;                         /* window positions that must hold a map pixel before a point is judged */
  int keep_classes;                        /* bit (1 << class) set: masked_out keeps the points of that class; 0 .. 15 */
} msfl_novelty_config;

/* msfl_carve_default_config with a window of 2 x 1 pixels, min_support = 1, keep = NONE | UNSEEN | COVERED. */
void msfl_novelty_default_config(msfl_novelty_config* cfg);

typedef struct msfl_novelty_info {
  int n_class[4];                          /* points per class, MSFL_NOV_NONE .. MSFL_NOV_IN_FRONT; their sum is n */
  int n_map_pixels;                        /* non-empty pixels of the image the labels were taken against */
  int n_kept;                              /* points whose class is in keep_classes */
  int applied;                             /* 1; 0 when msfl_grids_scan_novelty's device-resident pose was refused */
  int reserved_;
} msfl_novelty_info;

/* n == 0 is a scan that saw nothing: the counts are zero, MSFL_OK. */
msfl_status msfl_scan_novelty(msfl_handle* h, const msfl_point* scan, int n, const float* map_img, const msfl_novelty_config* cfg,
                              uint8_t* cls_out, msfl_point* masked_out, msfl_novelty_info* info, msfl_mem mem);

/* The chain in one call: msfl_grid_render of grids[0] with accumulate = 0, of grids[1 .. n_grids - 1] with accumulate = 1, all with
   cfg->image at pose7, then msfl_scan_novelty against that image; every output byte is what a caller chaining the public calls gets.
   n_grids in [1, 8], all grids of one handle (anything else: MSFL_BAD_ARG).  map_img_out: NULL, or n_row x n_col floats that receive
   the image.  A device-resident pose that is not finite: the image is all +inf, every point is MSFL_NOV_NONE, info->applied = 0. */
msfl_status msfl_grids_scan_novelty(msfl_grid* const* grids, int n_grids, const msfl_point* scan, int n, const double pose7[7],
                                    const msfl_novelty_config* cfg, uint8_t* cls_out, msfl_point* masked_out, float* map_img_out,
                                    msfl_novelty_info* info, msfl_mem mem);


/* ------------------------------------------------------------------------------------------ */
/* Scan segmentation: ground and range-image clusters before extraction (after LeGO-LOAM).      */
/* ------------------------------------------------------------------------------------------ */

/* msfl_segment_scans lays every sweep of a batch into its range image, takes the ground out by the slope between neighbouring beams,
   connects the remaining pixels into clusters by an angle test between neighbours and classifies every input point; the masked copy
   of the cloud (dropped points set to NaN) goes straight into msfl_extract_features* or msfl_slam_add_scan, whose invalid-point pass
   removes them.  docs/kernels/segment.md has the definition in full; every step is f32 with contraction off against the host-built
   tables of msfl_segment_tables, and every decision is an integer one after that, so numpy reproduces every output.  In short:
     pixel      row = the point's ring, column by bisection (column c covers the azimuths [2 pi (c - 1/2) / n_col, 2 pi (c + 1/2) / n_col):
                the columns are centred on the beams of a spinning sensor).  No pixel (class NONE): a point that is not finite, on the
                axis (x*x + y*y == 0), with !(r >= min_range) || r > max_range, or with ring >= n_row.  The pixel's winner is the point
                with the smallest (bits(r), index in its scan); every other point of the pixel is SHADOWED.
     ground     for every column and every k < ground_rows with pixels (k, col) and (k+1, col) both occupied, d = upper - lower winner:
                both are GROUND iff v*v <= g2 * n2, v = ((up.x*dx) + (up.y*dy)) + (up.z*dz), n2 = ((dx*dx) + (dy*dy)) + (dz*dz).
     edges      between occupied pixels that are not ground, 4-neighbourhood, columns wrap, rows do not: with d1 = fmaxf(ra, rb) and
                d2 = fminf(ra, rb) of the two winners' ranges, connected iff d2 * s > t * (d1 - d2 * c).
     components the transitive closure of the edges; a component's id is its smallest pixel index row * n_col + col.
     clusters   a component is valid iff count >= min_points, or count >= min_points_tall and it touches >= min_rows_tall rows.
     per point  SEGMENT / OUTLIER: the winner of a pixel of a valid / invalid component. */
enum { MSFL_SEG_NONE = 0, MSFL_SEG_SHADOWED = 1, MSFL_SEG_GROUND = 2, MSFL_SEG_SEGMENT = 3, MSFL_SEG_OUTLIER = 4, MSFL_SEG_CLASSES = 5 };

typedef struct msfl_segment_config {
  int n_col, n_row;                        /* columns of the full turn (even, 4..2048); rows = rings (2..128) */
  float elev_low_deg, elev_high_deg;       /* elevation of row 0 and of row n_row - 1, uniform in between: -90 < low < high < 90 */
  const float* row_elev_deg;               /* NULL, or a HOST array of n_row strictly ascending elevations in (-90, 90): uneven beams */
  float min_range, max_range;              /* metres, 0 <= min_range < max_range */
  int ground_rows;                         /* row pairs (k, k+1), k < ground_rows <= n_row - 1, that are tested; 0: no ground step */
  float ground_angle_deg;                  /* in (0, 90) */
  float up[3];                             /* the up direction in the sensor frame, a unit vector (|up|^2 within 1e-3 of 1) */
  float segment_angle_deg;                 /* in (0, 90) */
  int min_points, min_points_tall, min_rows_tall;   /* the cluster rule, each >= 1 */
  int keep_classes;                        /* bit (1 << class) set: masked_out keeps the points of that class; 0 .. 31 */
} msfl_segment_config;

/* The synthetic 16-beam sensor and LeGO-LOAM's published values: 1800 x 16 pixels, -15 .. +15 degrees, 0.3 .. 100 m, 8 ground row
   pairs, ground angle 10 degrees, up = (0, 0, 1), segment angle 60 degrees, cluster sizes 30 / 5 / 3, keep = GROUND | SEGMENT. */
void msfl_segment_default_config(msfl_segment_config* cfg);

/* The f32 tables the kernels compare against, built in double and rounded to f32 (pure host function, no handle):
     cc[k], cs[k] = cos, sin(2 pi (k - 1/2) / n_col), k < n_col / 2       the column boundaries of the half turn
     vs[k], vc[k] = sin, cos(e[k+1] - e[k]), k < n_row - 1                the elevation step of row pair k, e in radians
     scalars      = { sin, cos(2 pi / n_col), g2 = sin^2(ground_angle), t = tan(segment_angle) }
   with e[k] = row_elev_deg[k], or elev_low_deg + (elev_high_deg - elev_low_deg) k / (n_row - 1).
   MSFL_BAD_ARG: a null pointer, a configuration outside the limits above or with a field that is not finite. */
msfl_status msfl_segment_tables(const msfl_segment_config* cfg, float* cc, float* cs, float* vs, float* vc, float scalars[4]);

typedef struct msfl_segment_info {
  int n_class[5];                          /* points per class, MSFL_SEG_NONE .. MSFL_SEG_OUTLIER; their sum is the scan's n */
  int n_pixels;                            /* occupied pixels */
  int n_components;                        /* components among the occupied pixels that are not ground */
  int n_segments;                          /* valid components */
  int n_kept;                              /* points whose class is in keep_classes */
  int reserved_;
} msfl_segment_info;

/* Scan s is the region [off[s], off[s+1]) of pts / ring and of every output (`off`: HOST, n_scans + 1, never descending, off[0] >= 0;
   a point's index in its scan is its position minus off[s]).
     pts, ring   : sensor clouds as the driver delivers them (what msfl_extract_features_batch takes).
     cls_out     : one uint8_t per point, its class.
     segment_out : NULL, or one int per point: the component id for SEGMENT and OUTLIER, -1 otherwise.
     masked_out  : NULL, or one point per point: pts[i] when keep_classes has its class, else x = y = z = NaN and the fourth field
                   untouched.  Must not overlap pts.
     info        : NULL, or n_scans HOST records.  NULL: the call is stream-ordered and never waits for the device (device memory), so
                   masked_out can go into the next call as it is.  Non-NULL: the call reads the counts back (it synchronises).
     cfg         : NULL = msfl_segment_default_config.  HOST data, as is its row_elev_deg.
   With MSFL_MEM_DEVICE pts, ring and the three outputs are device pointers.  A batch whose images exceed the scratch budget is processed
   in chunks of scans on the stream; the results do not depend on the chunking.
   MSFL_BAD_ARG, before anything is staged or launched: n_scans < 0, off NULL or descending or off[0] < 0, pts / ring / cls_out NULL with
   points to process, masked_out overlapping pts, a configuration outside its limits. */
msfl_status msfl_segment_scans(msfl_handle* h, int n_scans, const msfl_point* pts, const uint16_t* ring, const int* off,
                               const msfl_segment_config* cfg, uint8_t* cls_out, int* segment_out, msfl_point* masked_out,
                               msfl_segment_info* info, msfl_mem mem);

/* The batch call with one scan of n points (info: NULL or one record). */
msfl_status msfl_segment_scan(msfl_handle* h, const msfl_point* pts, const uint16_t* ring, int n, const msfl_segment_config* cfg,
                              uint8_t* cls_out, int* segment_out, msfl_point* masked_out, msfl_segment_info* info, msfl_mem mem);


/* ------------------------------------------------------------------------------------------ */
/* The per-scan SLAM step, device-resident (BASELINE configs[2]: sequential odometry + mapping).*/
/*   replaces, for one incoming scan, the chain the reference runs across its two threads:      */
/*     RealHandleLaserCloudMessage   feature extraction            msf_loam_node.cc:160-378      */
/*     LaserOdometry::AddLaserScan   MatchScan2Scan + pose chain   laser_odometry.cc:69-95       */
/*     LaserMapping::Run             TransformAssociateToMap, MatchScan2Map (voxel filters,      */
/*                                   GetSurroundedCloud x2, gate, scan-to-map), TransformUpdate, */
/*                                   InsertScan2Map x2             laser_mapping.cc:138-258,260-338 */
/*   msfl_slam_add_scan is the LiDAR-only form (no IMU data: nothing to de-skew with);           */
/*   msfl_slam_add_scan_imu takes the per-scan IMU inputs and runs what LaserMapping::Run runs    */
/*   with them: UndistortScan before the match while the estimator is not initialised             */
/*   (laser_mapping.cc:170-176), the is_initialized matcher branch from the pre-solved pose        */
/*   (mapping_scan_matcher.cc:28-59,100-121) + DoUndistort before the insert (:197-211) once it is.*/
/* Raw points in, poses out: every intermediate (features, down-sampled clouds, the surrounded    */
/* map clouds, their kNN index, the two HybridGrid stores, the pose chain) stays in HBM, all        */
/* sizes are read by the kernels from device memory, and nothing synchronises with the host        */
/* between the upload of the scan and the 480-byte result record.  Like the reference's two        */
/* threads, the odometry chain of scan k+1 (one HIP stream) overlaps the mapping chain of scan k   */
/* (another stream; its corner side and the two voxel filters run on two more) when the caller     */
/* does not wait for every result.                                                                 */
/* ------------------------------------------------------------------------------------------ */

typedef struct msfl_slam_s msfl_slam;

typedef struct msfl_slam_config {
  float  map_resolution;      /* HybridGrid(3.0)                         laser_mapping.cc:44-45 */
  float  leaf_corner;         /* downsize_filter_corner_ 0.2             :60-63 */
  float  leaf_surf;           /* downsize_filter_surf_   0.4             :64-68 */
  int    min_map_corner;      /* MatchScan2Map runs iff corner > 10 ...  :284 */
  int    min_map_surf;        /* ... && surf > 50                        :285 */
  int    max_scan_points;     /* largest scan add_scan will see (capacity of the device buffers), e.g. 28 800 for a VLP-16 */
  int    max_rings;           /* rings of the sensor (16 / 64 / 128): bounds the per-scan sharp / flat counts the launches are sized for */
  double pose_odom2map[7];    /* initial pose_odom2map_ (identity in the reference, laser_mapping.h:88) */
  /* 0 (default): the mapping thread works on the scan's whole less-flat cloud, which is what FilterLessFlatLessCornerFeature
        (laser_mapping.cc:186,340-364) evidently means to do.
     1: reproduce what that function DOES: it copies cloud_surf_less_flat through the index list of the CORNER filter
        (`indices = downsize_filter_corner_.getIndices()` at :359 after the surf filter ran), i.e. the surf cloud is cut to its
        first n_less_sharp points, and that truncated cloud is what is voxel-filtered, used for GetSurroundedCloud, matched AND
        inserted into the map.  Use it to compare trajectories / maps with the real binary.  A scan with MORE less-sharp than
        less-flat points makes the reference read out of bounds (pcl::copyPointCloud); here: status_mapping = MSFL_BAD_ARG,
        status_imu untouched, the scan is neither matched nor inserted. */
  int    reference_quirks;
  /* 1: also produce the data products of LaserMapping::Run that reach neither the pose nor the map (round 5): cloud_full_res after
        the scan's IMU passes (UndistortScan :170-176 while not initialised, DoUndistort :206 once it is; untouched without IMU data)
        and its copy in the map frame, TransformPointCloud(cloud_full_res, pose_map_scan2world_) (:214-217: what the reference
        accumulates for its PLY dump and publishes), fetched with msfl_slam_get_clouds; the sharp / flat / less-sharp / less-flat
        clouds of PublishScan (:418-440) are index lists into that cloud.  One more launch per scan.  0 (default): not computed. */
  int    keep_clouds;
} msfl_slam_config;

typedef struct msfl_slam_result {
  double pose_odom[7];        /* pose_scan2world_ of the odometry thread (laser_odometry.cc:79), odometry frame */
  double pose_map[7];         /* pose_map_scan2world_ after MatchScan2Map (laser_mapping.cc:304-311): the SLAM output */
  double pose_curr2last[7];   /* pose_curr2last_ (laser_odometry.cc:75) */
  double pose_odom2map[7];    /* pose_odom2map_ after TransformUpdate (laser_mapping.h:59-61) */
  msfl_match_info odometry;   /* MatchScan2Scan diagnostics (status MSFL_TOO_FEW_CORRESPONDENCES where the reference returns false) */
  msfl_match_info mapping;    /* MatchScan2Map diagnostics (all zero when the gate was closed) */
  int scan_index;             /* 0-based count of add_scan calls */
  int status_extract;         /* msfl_status of the extraction (MSFL_BAD_RING, MSFL_CAPACITY, ...) */
  int status_mapping;         /* 0, or MSFL_MAP_TOO_SMALL when the gate (:284-285) kept MatchScan2Map from running,
                                 or MSFL_CAPACITY when a list did not fit the on-chip voxel filter */
  int n_full, n_sharp, n_less_sharp, n_flat, n_less_flat;   /* extraction counts */
  int n_corner_ds, n_surf_ds;           /* after the 0.2 / 0.4 m voxel filters (:264-270) */
  int n_map_corner, n_map_surf;         /* GetSurroundedCloud sizes (:273-278) */
  int grid_corner[8], grid_surf[8];     /* map store after the inserts: {points, cells, pool_top, dropped, overflow, cells touched, ...};
                                           on a scan that msfl_slam_set_map_window cropped, [0..2] are the sizes AFTER the crop */
  int status_imu;             /* 0, or MSFL_BAD_ARG: a less-sharp / less-flat point's relative time lies outside the scan's
                                 pre-integration span (GetDeltaQP CHECK-aborts there, scan_undistortion.cc:26-30; CHECK_GE(time, 0) :12):
                                 the scan is then neither matched nor inserted (status_mapping = MSFL_BAD_ARG as well) */
  int status_insert;          /* 0, or MSFL_CAPACITY: one of the two InsertScan calls was dropped (grid_*[3] / [4] != 0: a point outside
                                 the +-8192-cell range / not finite, or an internal capacity); the map store is then unchanged */
  int status_clouds;          /* keep_clouds: 0, or MSFL_BAD_ARG: a point of cloud_full_res OUTSIDE the less-sharp / less-flat lists (ring
                                 margins, corner neighbourhoods) has a relative time outside the pre-integration span; the reference
                                 CHECK-aborts on it inside UndistortScan / DoUndistort, here that point is left as it was */
  int reserved_;
} msfl_slam_result;

void msfl_slam_default_config(msfl_slam_config* c);

/* One SLAM pipeline = the reference's LaserOdometry + LaserMapping pair (four streams, the matchers' scratch, two map stores). */
msfl_status msfl_slam_create(const msfl_params* params, const msfl_slam_config* config, int device, msfl_slam** out);
void msfl_slam_destroy(msfl_slam* s);

/* Feed one scan as pcl::fromROSMsg delivers it (driver order, `n` points + ring ids).  With mem == MSFL_MEM_HOST the
   arrays are copied into pinned staging before the call returns; with MSFL_MEM_DEVICE they must stay untouched until
   this scan's result is out.
     result != NULL : wait for this scan's mapping result and deliver it (one synchronisation per scan);
     result == NULL : enqueue only; fetch the record later with msfl_slam_get_result.  At most two scans are in flight:
                      the call first waits for scan index-2 (almost always long done).
   Returns a status for argument / HIP errors only; per-scan outcomes are in the record. */
msfl_status msfl_slam_add_scan(msfl_slam* s, const msfl_point* pts, const uint16_t* ring, int n, msfl_mem mem,
                               msfl_slam_result* result);

/* Per-scan IMU inputs of LaserMapping::Run.  Everything here is produced by code OUTSIDE the hot path (IMU pre-integration,
   the estimator, the 15-residual IMU-only pre-solve: SURVEY.md 8f N3) and handed over like the reference's members:
     pre            BuildPreintegration(imu_buf_, odom_result.time) (laser_mapping.cc:191-194, :399); NULL = no IMU data for
                    this scan (the step then behaves like msfl_slam_add_scan, whatever is_initialized says)
     is_initialized estimator_.IsInitialized() (:173,:197; the reference switches after kInitByFirstScanNums = 50 scans, estimator.h:57)
       0: UndistortScan (:170-176 -> scan_undistortion.cc:5-19,45-62): p <- dq(p.time).cast<float>() * p on the clouds the mapping
          thread works with, BEFORE FilterLessFlatLessCornerFeature, the voxel filters, GetSurroundedCloud, the match and the insert;
          velocity / gravity / presolved_pose are not read
       1: the match starts from presolved_pose (pose_j of the IMU-only Ceres problem, mapping_scan_matcher.cc:35-59; the caller solves
          it, cf. MappingScanMatcher::SetImuPresolve in include/msfl/scan_matcher.hpp) and uses the Deskew factors with
          (dq, dp) = GetDeltaQP(pre, t) per down-sampled feature, Vi = velocity held constant (:94) and `gravity` (:100-121,154-166,
          224-236); afterwards DoUndistort (:197-211) rewrites the clouds that InsertScan2Map then inserts:
            p <- (dq(t) * p + pose_odom.rotation()^-1 * (velocity * t - 0.5 * gravity * t * t) + dp(t)).cast<float>()
          GetSurroundedCloud still uses TransformAssociateToMap's pose (:185,:273-278), like the reference.
   The odometry thread (MatchScan2Scan) never sees any of this: it works on the raw feature clouds (laser_odometry.cc:69-95).
   Which clouds: cloud_corner_less_sharp and cloud_surf_less_flat, the two that reach the pose and the map.  The reference also
   rewrites cloud_full_res (published / accumulated for the PLY dump only) and, in the not-initialised branch, the sharp / flat clouds,
   which nothing reads afterwards (FilterLessFlatLessCornerFeature hands on EMPTY sharp / flat clouds, :344-345): with
   msfl_slam_config.keep_clouds = 1 the step produces those too (msfl_slam_get_clouds).
   `pre` holds at most 2 048 samples (MSFL_CAPACITY beyond); the arrays are copied before the call returns. */
typedef struct msfl_slam_imu {
  const msfl_preintegration* pre;
  int    is_initialized;
  double velocity[3];         /* velocity_ = bias_j.head<3>() of the pre-solve (mapping_scan_matcher.cc:58) */
  double gravity[3];          /* estimator_.GetGravityVector() */
  double presolved_pose[7];   /* pose_j (:57) */
} msfl_slam_imu;

/* msfl_slam_add_scan with the scan's IMU inputs (imu == NULL: identical to msfl_slam_add_scan).  With is_initialized = 1 the
   pre-solve needs the previous scan's mapping result, so a caller normally fetches that result before feeding the next scan. */
msfl_status msfl_slam_add_scan_imu(msfl_slam* s, const msfl_point* pts, const uint16_t* ring, int n, msfl_mem mem,
                                   const msfl_slam_imu* imu, msfl_slam_result* result);

/* Wait for the scan with the given index (one of the last four fed) and deliver its record. */
msfl_status msfl_slam_get_result(msfl_slam* s, int scan_index, msfl_slam_result* result);

/* Uncertainty of the two registrations of every scan fed from now on (enabled != 0), see msfl_match_uncertainty; min_eigenvalue as
   in msfl_set_uncertainty.  Results (msfl_slam_result) are bit-identical with the feature on and off. */
msfl_status msfl_slam_set_uncertainty(msfl_slam* s, int enabled, double min_eigenvalue);
/* The records of scan `scan_index` (one of the last four fed, like msfl_slam_get_result; waits for it): MatchScan2Scan's and
   MatchScan2Map's.  Either pointer may be NULL.  odometry->valid == 0 for scan 0 and where MatchScan2Scan returned false;
   mapping->valid == 0 when the gate (min_map_corner / min_map_surf) kept the match from running.  MSFL_BAD_ARG for a scan that
   was fed while the feature was off. */
msfl_status msfl_slam_get_uncertainty(msfl_slam* s, int scan_index, msfl_match_uncertainty* odometry, msfl_match_uncertainty* mapping);

/* Degeneracy-aware solve (msfl_set_degeneracy) of the two registrations of every scan fed from now on: `odometry` switches
   MatchScan2Scan's solves, `mapping` MatchScan2Map's, each with a threshold of its own (their information matrices live on
   different scales).  With both 0 the feature is off.  MSFL_BAD_ARG for a negative or non-finite threshold of a matcher that is
   switched on.  Where nothing is held the results (msfl_slam_result) are bit-identical to a run without the feature. */
msfl_status msfl_slam_set_degeneracy(msfl_slam* s, int odometry, int mapping, double min_eig_odometry, double min_eig_mapping);
/* The records of scan `scan_index`, under the rules of msfl_slam_get_uncertainty (one of the last four fed; waits for it; either
   pointer may be NULL; MSFL_BAD_ARG for a scan that was fed while both switches were off).  A matcher that was off, or did not
   run, leaves its record all zero. */
msfl_status msfl_slam_get_degeneracy(msfl_slam* s, int scan_index, msfl_degeneracy_record* odometry, msfl_degeneracy_record* mapping);

/* Outlier rejection (msfl_set_outlier_rejection) of the two registrations of every scan fed from now on: `odometry` configures
   MatchScan2Scan's solves, `mapping` MatchScan2Map's; NULL (or mode MSFL_REJECT_OFF) leaves that matcher without it.  The
   reference tests odom_min_correspondences before its (commented-out) rejection call; here the survivors decide.
   MSFL_BAD_ARG under the rules of msfl_set_outlier_rejection. */
msfl_status msfl_slam_set_outlier_rejection(msfl_slam* s, const msfl_outlier_rejection* odometry, const msfl_outlier_rejection* mapping);
/* The records of scan `scan_index`, under the rules of msfl_slam_get_degeneracy (MSFL_BAD_ARG for a scan that was fed while both
   matchers had the feature off).  A matcher that was off, or did not run, leaves its record all zero. */
msfl_status msfl_slam_get_rejection(msfl_slam* s, int scan_index, msfl_rejection_record* odometry, msfl_rejection_record* mapping);

/* Pose priors for the NEXT msfl_slam_add_scan[_imu] only (host pointers, copied here; either may be NULL = none):
     odometry : on that scan's MatchScan2Scan, whose unknown is the RELATIVE pose pose_curr2last;
     mapping  : on its scan-to-map solve, whose unknown is the WORLD pose pose_map (a GPS fix, an IMU-predicted pose).
   The records travel with the scan that consumes them, so feeding further scans while that one is still queued is safe.
   MSFL_BAD_ARG for a non-finite entry (nothing is changed then). */
msfl_status msfl_slam_set_next_prior(msfl_slam* s, const msfl_pose_prior* odometry, const msfl_pose_prior* mapping);

/* Windowed local map (see msfl_grid_crop): from the next scan fed on, after the two InsertScan calls of every scan with
   (scan_index + 1) % every_n_scans == 0 both stores are cropped to +-half_cells cells around the translation of that scan's
   pose_map, on the device and without a synchronisation.  half_cells == NULL turns the window off (the default; every_n_scans is
   then ignored).  The evicted points are dropped: a caller who wants the global map keeps msfl_slam_config.keep_clouds and
   accumulates full_map, the map-frame full cloud per scan, which is what the reference accumulates for its PLY dump
   (laser_mapping.cc:214-217).  On a cropped scan grid_corner[0..2] / grid_surf[0..2] of the record are the sizes after the crop.
   With a window of at least 23 cells of 3 m per axis and a sensor range inside it, poses and records are bit-identical to a run
   without the window (see msfl_grid_crop for longer ranges).  MSFL_BAD_ARG: a negative entry, every_n_scans < 1. */
msfl_status msfl_slam_set_map_window(msfl_slam* s, const int half_cells[3], int every_n_scans);
/* What the crops of scan `scan_index` (one of the last four fed; waits for it) did to the corner / surf store.  Either pointer may
   be NULL.  All-zero records for a scan on which no crop ran. */
msfl_status msfl_slam_get_map_window(msfl_slam* s, int scan_index, msfl_grid_crop_info* corner, msfl_grid_crop_info* surf);

/* msfl_slam_config.keep_clouds: the clouds of scan `scan_index` (it must be one of the last TWO fed: the buffers belong to a set that
   the scan after next reuses).  Waits for that scan's chain.
     mem == MSFL_MEM_DEVICE: the function FILLS the pointers with device addresses (valid until msfl_slam_add_scan of scan_index + 2);
     mem == MSFL_MEM_HOST  : the CALLER fills the pointers it wants (NULL = not wanted) with host arrays of max_scan_points elements
                             each and the function copies.
   Counts are always delivered.  index lists address points of `full_scan` / `full_map` / `ring`. */
typedef struct msfl_slam_clouds {
  msfl_point* full_scan;      /* cloud_full_res in the scan frame after the IMU passes of LaserMapping::Run (:170-176,:206) */
  msfl_point* full_map;       /* TransformPointCloud(cloud_full_res, pose_map_scan2world_) (:214-217), f32 */
  uint16_t*   ring;           /* ring id of every point of the full cloud */
  int *sharp_idx, *less_sharp_idx, *flat_idx, *less_flat_idx;   /* msf_loam_node.cc:279-344 as positions in the full cloud */
  int n_full, n_sharp, n_less_sharp, n_flat, n_less_flat;
} msfl_slam_clouds;
msfl_status msfl_slam_get_clouds(msfl_slam* s, int scan_index, msfl_slam_clouds* clouds, msfl_mem mem);

/* The two map stores (hybrid_grid_map_corner_ / hybrid_grid_map_surf_), e.g. for msfl_grid_dump at shutdown
   (laser_mapping.cc:95-113).  Owned by the pipeline; do not destroy.  Waits for everything in flight. */
msfl_status msfl_slam_grids(msfl_slam* s, msfl_grid** corner, msfl_grid** surf);
const char* msfl_slam_last_error(const msfl_slam* s);

/* ------------------------------------------------------------------------------------------------------------------
   Place recognition: a device-resident database of polar scan descriptors (after Scan Context, Kim & Kim 2018) that
   answers "which earlier scan looks like this one, and at which yaw".  docs/kernels/place.md holds the full definition;
   in short, all f32 against tables the host builds once in double and rounds to f32
   (e2[k] = (k max_range / n_ring)^2, lo2 = min_range^2, bc/bs[k] = cos/sin(2 pi k / n_sector)):
     - a point with a non-finite coordinate is skipped; r2 = x*x + y*y; skipped unless lo2 <= r2 < e2[n_ring];
     - ring = #{k in [1, n_ring) : r2 >= e2[k]};  the point is mirrored through the origin into the upper half plane
       (y > 0, or y == 0 and x > 0) and sector = (mirrored ? n_sector/2 : 0) + #{k in [1, n_sector/2) : bc[k] y' - bs[k] x' >= 0};
     - v = z + (float)height_offset, skipped unless v > 0;  D[ring][sector] = max(D[ring][sector], v), starting from 0.
   Per entry: ring_key[r] = number of sectors with D[r][s] > 0; column norms in f64.
   Distance of query q to entry c at shift s (column j of q against column (j + s) mod n_sector of c): the mean over the
   columns j with both norms > 0 of 1 - dot_j / (|q_j| |c_j+s|), in f64 with ascending summation; +inf without such a
   column.  A result carries the minimum over s and the lowest s that attains it: the yaw between the two visits in steps
   of 2 pi / n_sector.  Every sum has one stated order: results do not depend on batch shape or launch shape.
   The object owns a stream and its memory and is independent of msfl_handle and msfl_slam. */
typedef struct msfl_place_config {
  int n_ring;            /* 1 .. 32   (default 20) */
  int n_sector;          /* 2 .. 120, even (default 60) */
  double min_range;      /* 0 <= min_range < max_range (defaults 0.3, 80.0), metres in the scan's xy plane */
  double max_range;
  double height_offset;  /* added to z, so that heights are positive: roughly the sensor's height above ground (default 2.0) */
  int capacity;          /* entries the database can hold, fixed at creation (default 16384) */
} msfl_place_config;

typedef struct msfl_place_match {
  int index;             /* entry, -1 in an unused slot */
  int shift;             /* columns; see above */
  int ring_key_d2;       /* squared distance of the two ring keys */
  int n_columns;         /* columns that entered the mean at `shift` */
  double distance;       /* +inf in an unused slot and for a descriptor without a common column */
} msfl_place_match;

typedef struct msfl_places_s msfl_places;
/* MSFL_BAD_ARG for a config outside the limits above, a non-finite value or capacity < 1.  NULL config = defaults. */
void        msfl_places_default_config(msfl_place_config* c);
msfl_status msfl_places_create(const msfl_place_config* c, int device, msfl_places** out);
void        msfl_places_destroy(msfl_places* p);
msfl_status msfl_places_set_stream(msfl_places* p, void* hip_stream);   /* as msfl_set_stream */
msfl_status msfl_places_synchronize(msfl_places* p);
int         msfl_places_size(const msfl_places* p);                     /* entries added so far (host count) */
const char* msfl_places_last_error(const msfl_places* p);
/* Rules for the calls below:
     - MSFL_CAPACITY when an add would exceed `capacity`: nothing is added, not even part of the batch.
     - MSFL_BAD_ARG: k < 1 or k > 64, n_prefilter < 0, decreasing offsets, an entry index that is no entry, a max_index
       outside [0, size], descriptors with a value that is negative or not finite (host memory: checked before staging; device
       memory: checked on the device, which waits for the stream; the whole add is refused).
     - A scan with no binnable point is a valid all-zero entry; its distance to anything is +inf.
     - Offsets, entry lists and max_index are HOST arrays.  With MSFL_MEM_DEVICE clouds, descriptors and results are device
       pointers (16-byte aligned points) and the call is asynchronous on the object's stream: a query after an add sees the
       new entries.  msfl_slam_get_clouds(..., MSFL_MEM_DEVICE).full_scan can be handed over as it is.
     - Candidates of query i are the entries below max_index[i] (NULL: every entry present when the call is enqueued).
       n_prefilter == 0 compares all of them; n_prefilter > 0 only the n_prefilter with the smallest ring_key_d2, ties to the
       lowest index.  Results: k records per query ordered by (distance, index), unused slots {-1, 0, 0, 0, +inf}. */
/* describe n_scans scans (concatenated points + n_scans+1 HOST prefix offsets) and append them; *first_index = index of the first */
msfl_status msfl_places_add(msfl_places* p, const msfl_point* pts, const int* off, int n_scans, msfl_mem mem, int* first_index);
/* append n ready descriptors (n x n_ring x n_sector f32, row-major [ring][sector]) - what msfl_places_get delivered; keys and norms are recomputed */
msfl_status msfl_places_add_descriptors(msfl_places* p, const float* desc, int n, msfl_mem mem, int* first_index);
msfl_status msfl_places_get(msfl_places* p, int first, int n, float* desc_out, int* ring_key_out /* n x n_ring, may be NULL */, msfl_mem mem);
msfl_status msfl_places_query(msfl_places* p, const msfl_point* pts, const int* off, int n_queries, const int* max_index,
                              int n_prefilter, int k, msfl_place_match* out /* n_queries x k */, msfl_mem mem);
msfl_status msfl_places_query_entries(msfl_places* p, const int* entries /* HOST */, int n_queries, const int* max_index,
                                      int n_prefilter, int k, msfl_place_match* out, msfl_mem mem);

/* ------------------------------------------------------------------------------------------------------------------
   Pose-graph optimisation: what GpsFusion::Optimize (src/slam/gps_fusion/gps_fusion.cc:27-97) does with Ceres, and
   what a loop closer does with an accepted closure (loop_closure/pose_graph_factor.h), on the device.
   docs/kernels/graph.md holds the full definition; in short, all f64:
     - nodes are poses [t(3), qx qy qz qw];
     - a relative-pose edge {i, j, z, sr, st} (RelativePoseFactor, gps_factor.h:36-48): T_ij = T_i^-1 T_j, E = T_ij^-1 Z,
       r = [E.t / st ; vec(E.q) / sr], 6 rows; the quaternion is used as it comes out, without sign normalisation;
     - a position fix {i, j, t, p, st} (GpsFactor, gps_factor.h:12-17): r = ((1 - t) t_i + t t_j - p) / st, 3 rows;
     - HuberLoss(huber_delta) on each block's squared norm through Ceres' corrector (rho'' <= 0 branch); 0 = no loss;
     - per free node t + dt and EigenQuaternionParameterization, q <- dq (x) q, dq = [sin|d| d/|d| ; cos|d|] (identity at
       d = 0); nodes marked fixed are no variables and enter neither the tangent vector nor x_norm;
     - the solve is Ceres 1.14's TrustRegionMinimizer with LEVENBERG_MARQUARDT over the stacked tangent of all free nodes:
       Jacobi scaling fixed after iteration 0, LM diagonal clipped to [min_lm_diagonal, max_lm_diagonal], the step the
       solution of (Js^T Js + D^2) s = -Js^T r;
     - that system is solved by conjugate gradients to cg_tolerance (relative, in the preconditioner norm), preconditioned
       by the exact solve of its block-tridiagonal part (block pairs |i - j| <= 1 in the numbering of the free nodes); the
       remaining blocks, those of the LONG factors (both ends free, more than one apart), enter through the mat-vec.
       Without a long factor the preconditioner's solve is the step and exactly one CG iteration runs per LM iteration.
       With long factors at most max_cg_iterations run (0: 16 n_long + 8); a solve that ends there hands over its iterate
       and counts in cg_unconverged.
     - information-weighted forms of both factors (msfl_graph_edge_info, msfl_graph_fix_info, further down) carry a full
       square-root information matrix, built from a registration's msfl_match_uncertainty or a 3 x 3 covariance by
       msfl_graph_edge_from_uncertainty / msfl_graph_fix_from_covariance; msfl_graph_factor_chi2 reads |r|^2 per factor back.
   Every sum has one stated order (factors per node in the order edges were added, then fixes, then information edges, then
   information fixes; totals over fixed-size
   partials in index order) and there are no floating-point atomics: the same records in the same order give the same
   bits, however the add_* calls were chunked.  The object owns a stream and its memory, like msfl_places. */
typedef struct msfl_graph_config {
  int max_nodes, max_edges, max_fixes;      /* capacities, fixed at creation (defaults 16384, 32768, 16384) */
  int max_num_iterations;                   /* 10 (gps_fusion.cc:45) */
  int max_consecutive_invalid_steps;        /* 5 */
  int jacobi_scaling;                       /* 1 */
  int max_cg_iterations;                    /* 0 = 16 n_long + 8 */
  int reserved;
  double huber_delta;                       /* 1.0 (gps_fusion.cc:48); 0 = no loss */
  double initial_trust_region_radius, max_trust_region_radius, min_trust_region_radius;   /* 1e4, 1e16, 1e-32 */
  double min_relative_decrease;             /* 1e-3 */
  double min_lm_diagonal, max_lm_diagonal;  /* 1e-6, 1e32 */
  double function_tolerance, gradient_tolerance, parameter_tolerance;                      /* 1e-6, 1e-10, 1e-8 */
  double cg_tolerance;                      /* 1e-12 */
} msfl_graph_config;

typedef struct msfl_graph_edge { int i, j; double z[7]; double sr, st; } msfl_graph_edge;          /* z = the measured T_i^-1 T_j */
typedef struct msfl_graph_fix { int i, j; double t; double p[3]; double st; } msfl_graph_fix;

enum { MSFL_GRAPH_EMPTY = 0, MSFL_GRAPH_GRADIENT = 1, MSFL_GRAPH_MAX_ITERATIONS = 2, MSFL_GRAPH_MIN_RADIUS = 3,
       MSFL_GRAPH_INVALID_STEPS = 4, MSFL_GRAPH_PARAMETER = 5, MSFL_GRAPH_FUNCTION = 6 };

typedef struct msfl_graph_summary {
  int status;                /* msfl_status of the solve */
  int termination;           /* MSFL_GRAPH_*: why the minimizer stopped */
  int iterations;            /* LM iterations (steps tried) */
  int successful_steps;
  double initial_cost, final_cost;
  int cg_iterations;         /* in total over all LM iterations */
  int cg_unconverged;        /* step solves that ended at max_cg_iterations */
  int n_long_edges;          /* long factors (edges or fixes) */
  int n_free;                /* free nodes */
} msfl_graph_summary;

typedef struct msfl_graph_s msfl_graph;
/* MSFL_BAD_ARG for a config with a negative or non-finite value or max_nodes < 1.  NULL config = defaults. */
void        msfl_graph_default_config(msfl_graph_config* c);
msfl_status msfl_graph_create(const msfl_graph_config* c, int device, msfl_graph** out);
void        msfl_graph_destroy(msfl_graph* g);
msfl_status msfl_graph_set_stream(msfl_graph* g, void* hip_stream);   /* as msfl_set_stream */
msfl_status msfl_graph_synchronize(msfl_graph* g);
const char* msfl_graph_last_error(const msfl_graph* g);
msfl_status msfl_graph_clear(msfl_graph* g);                          /* no nodes, edges or fixes; capacities stay */
int         msfl_graph_num_nodes(const msfl_graph* g);
/* Building.  Refusals leave the graph as it was and set last_error:
     - MSFL_BAD_ARG: a node index out of range; i == j; a non-finite value; sr, st <= 0; t outside [0, 1]; a zero quaternion
       (in a pose or in z);
     - MSFL_CAPACITY: the call would exceed max_nodes / max_edges / max_fixes; the whole call is refused, not part of it.
   Edge and fix records are HOST arrays (the host keeps the structure: adjacency lists and launch sizes).  Poses may be
   device memory (MSFL_MEM_DEVICE: double[7] per node; the call checks them on the host, so it waits for the stream);
   msfl_slam results can be handed over as they are. */
msfl_status msfl_graph_add_nodes(msfl_graph* g, const double* poses, int n, msfl_mem mem, int* first_index);
msfl_status msfl_graph_add_edges(msfl_graph* g, const msfl_graph_edge* edges /* HOST */, int n);
msfl_status msfl_graph_add_fixes(msfl_graph* g, const msfl_graph_fix* fixes /* HOST */, int n);
msfl_status msfl_graph_set_fixed(msfl_graph* g, int node, int flag);  /* SetParameterBlockConstant / ...Variable */
msfl_status msfl_graph_set_poses(msfl_graph* g, int first, int n, const double* poses, msfl_mem mem);
msfl_status msfl_graph_get_poses(msfl_graph* g, int first, int n, double* out, msfl_mem mem);
/* cost = 1/2 sum rho(|r|^2) at the current poses; changes nothing */
msfl_status msfl_graph_cost(msfl_graph* g, double* cost);
/* Synchronous.  Reads one small record from the device per LM iteration, none per CG iteration or reduction level.  The
   poses afterwards are the last accepted iterate.  Without a free node or without a factor: termination
   MSFL_GRAPH_EMPTY, poses untouched. */
msfl_status msfl_graph_optimize(msfl_graph* g, msfl_graph_summary* summary);
/* the last optimize, per LM iteration: accepted[k] = 1 accepted, 0 rejected (or the tolerance test that ended the solve), -1 an
   invalid step; cost[k] = the candidate's cost.  *n_out = iterations recorded; MSFL_CAPACITY if that exceeds `capacity`
   (the first `capacity` are written).  Either array may be NULL. */
msfl_status msfl_graph_get_trace(msfl_graph* g, int* accepted, double* cost, int capacity, int* n_out);

/* Information-weighted factors: the two kinds above with a full square-root information matrix L (row-major, information =
   L^T L, any rank but zero) in place of the scalar sigmas.  The residual is the pose prior's (msfl_pose_prior) applied to the
   relative pose:
     edge: T_ij = T_i^-1 T_j;  qe = conj(z.q) (x) q_ij, negated when qe.w < 0;  e = [t_ij - z.t ; 2 qe.xyz];  r = L e   (6 rows)
     fix:  r = L3 ((1 - t) t_i + t t_j - p)                                                                          (3 rows)
   so L^T L is the inverse covariance of the measurement z in the tangent [dt ; dtheta] with z.t + dt, z.q (x) dq(dtheta): the
   tangent convention of msfl_match_uncertainty.information.  A zero row of L is a direction the factor does not pull along.
   HuberLoss(huber_delta) applies to |r|^2 as for the other kinds.  With L = diag(1/st x 3, 1/(2 sr) x 3) the cost of an
   information edge equals that of msfl_graph_edge {sr, st} at any poses (the Jacobians differ: the old residual is T_ij^-1 Z,
   this one Z^-1 T_ij).
   Factors are numbered edges, fixes, information edges, information fixes, each kind in the order added; sums per node follow
   that numbering.  Information edges count against max_edges together with plain edges, information fixes against max_fixes
   together with plain fixes.  A graph without an information factor launches and allocates nothing more than before.
   Refusals as for the plain adders; an L whose entries are all zero is MSFL_BAD_ARG too. */
typedef struct msfl_graph_edge_info { int i, j; double z[7]; double sqrt_information[36]; } msfl_graph_edge_info;   /* 352 bytes */
typedef struct msfl_graph_fix_info { int i, j; double t; double p[3]; double sqrt_information[9]; } msfl_graph_fix_info; /* 112 bytes */
msfl_status msfl_graph_add_edges_info(msfl_graph* g, const msfl_graph_edge_info* edges /* HOST */, int n);
msfl_status msfl_graph_add_fixes_info(msfl_graph* g, const msfl_graph_fix_info* fixes /* HOST */, int n);
/* From a registration to an edge; pure host arithmetic, no GPU call.  pose_j is the registered pose and `unc` its record
   (information about pose_j: t += dt in the parent frame, q = q dq(dtheta) in the body frame); pose_i is taken as exact.
   z = T_i^-1 T_j; row k of L is sqrt(eigenvalues[k] / scale) v_k^T diag(R_i, I) for k >= n_degenerate and zero below, so
   L^T L = diag(R_i^T, I) H_kept diag(R_i, I) / scale: a registration that is blind along a corridor gives an edge that does not
   pull along it.  `scale` is the variance factor (unc->sigma2, or a sensor model's), finite and > 0.  For a registration whose
   record is about the relative pose itself pass pose_i = identity and pose_j = the relative pose.  MSFL_BAD_ARG, *out
   untouched: unc->valid == 0, n_degenerate == 6, a non-finite input, a zero quaternion, i == j or a negative index. */
msfl_status msfl_graph_edge_from_uncertainty(int i, int j, const double pose_i[7], const double pose_j[7],
                                             const msfl_match_uncertainty* unc, double scale, msfl_graph_edge_info* out);
/* L3 = the upper Cholesky factor of covariance^-1 (row-major 3 x 3, as a GPS receiver reports it).  MSFL_BAD_ARG, *out
   untouched: a covariance that is not finite or not symmetric positive definite, t outside [0, 1], i == j. */
msfl_status msfl_graph_fix_from_covariance(int i, int j, double t, const double p[3], const double covariance[9],
                                           msfl_graph_fix_info* out);
/* |r|^2 of factors first .. first + n of one kind at the current poses, before the loss; changes nothing, like msfl_graph_cost.
   With information weights this is a chi-square with 6 (3 for a fix) degrees of freedom under the model: the number a loop
   closer thresholds on.  MSFL_BAD_ARG for an unknown kind or a range outside that kind's factors. */
enum { MSFL_GRAPH_FACTOR_EDGE = 0, MSFL_GRAPH_FACTOR_FIX = 1, MSFL_GRAPH_FACTOR_EDGE_INFO = 2, MSFL_GRAPH_FACTOR_FIX_INFO = 3 };
msfl_status msfl_graph_factor_chi2(msfl_graph* g, int kind, int first, int n, double* out /* HOST */);

/* A loss per factor (docs/kernels/graph.md, "A loss per factor"): Ceres gives every residual block a LossFunction of its own, and so
   does this.  A loop closer leaves the odometry chain at the graph's loss and puts a redescending one on its closures: a wrong
   closure is then switched off inside the solve, and msfl_graph_factor_weights reads the inlier decision back.  With s = |r|^2,
   a > 0, b = a^2 (Ceres' forms; every rho' is clamped from below at DBL_MIN):
     DEFAULT        the graph's huber_delta, what every factor has without a record
     NONE           rho = s                                  rho' = 1
     HUBER          rho = s if s <= b, else 2 a sqrt(s) - b  rho' = 1, else a / sqrt(s)
     SOFT_L_ONE     rho = 2 b (sqrt(1 + s/b) - 1)            rho' = 1 / sqrt(1 + s/b)
     CAUCHY         rho = b log(1 + s/b)                     rho' = 1 / (1 + s/b)
     GEMAN_MCCLURE  rho = b s / (b + s)                      rho' = (b / (b + s))^2
   All have rho'' <= 0: residual and Jacobian rows are scaled by sqrt(rho'), the cost is rho / 2, as for HuberLoss(huber_delta).
   msfl_graph_cost, msfl_graph_optimize and msfl_graph_marginals all see the records.
   set_losses gives factors first .. first + n of one factor kind (MSFL_GRAPH_FACTOR_*) the records losses[0 .. n_losses), n_losses
   = n, or 1 to give them all the same one.  It may be called again at any time for factors that exist (a shrinking-a schedule is a
   loop of set_losses and optimize in the caller).  `a` of DEFAULT and NONE is not read and is stored as 0.  Factors added later
   start at DEFAULT; msfl_graph_clear forgets the records.  MSFL_BAD_ARG, nothing set: an unknown factor or loss kind, a <= 0 or a
   non-finite a on a kind that reads it, a range outside that kind's factors, n_losses neither n nor 1.
   A graph that never calls set_losses allocates and launches nothing more than before and runs the same kernels. */
enum { MSFL_GRAPH_LOSS_DEFAULT = 0, MSFL_GRAPH_LOSS_NONE = 1, MSFL_GRAPH_LOSS_HUBER = 2, MSFL_GRAPH_LOSS_SOFT_L_ONE = 3,
       MSFL_GRAPH_LOSS_CAUCHY = 4, MSFL_GRAPH_LOSS_GEMAN_MCCLURE = 5 };
typedef struct msfl_graph_loss { int kind; int reserved; double a; } msfl_graph_loss;
msfl_status msfl_graph_set_losses(msfl_graph* g, int factor_kind, int first, int n, const msfl_graph_loss* losses /* HOST */,
                                  int n_losses);
/* the records of factors first .. first + n; a factor that was never given one reports DEFAULT */
msfl_status msfl_graph_get_losses(msfl_graph* g, int factor_kind, int first, int n, msfl_graph_loss* out /* HOST */);
/* rho'(|r|^2) of factors first .. first + n at the current poses, each under its own loss: 1 for a factor the loss leaves alone,
   towards 0 for one it has switched off.  Changes nothing and refuses what msfl_graph_factor_chi2 refuses. */
msfl_status msfl_graph_factor_weights(msfl_graph* g, int factor_kind, int first, int n, double* out /* HOST */);

/* Marginal and cross covariances of the poses (docs/kernels/graph.md, "Marginals"): what Ceres'
   Covariance::GetCovarianceBlockInTangentSpace gives.  At the current poses every factor is linearised as the solve linearises it
   (HuberLoss corrector at huber_delta applied), H = J^T J over the free nodes' tangent with NO LM diagonal, Sigma = H^-1.
   Tangent conventions of this header, all three:
     - msfl_match_uncertainty: t += dt in the parent frame, q = q dq(dtheta) in the body frame (right rotation);
     - msfl_graph_edge_info: z.t + dt, z.q (x) dq(dtheta), in the frame of node i;
     - these blocks: [dt ; dtheta] with t + dt and q <- dq(dtheta) (x) q, BOTH in the world frame (left rotation vector in radians).
       The solver's own tangent is [dt ; d] with dtheta = 2 d, so a delivered block is diag(I, 2I) Sigma_d diag(I, 2I).
   `pairs` holds n_pairs node pairs (a, b), any order, duplicates allowed; pair k gives out[36 k ..]: Sigma_ab row-major, rows of a,
   columns of b.  a == b is the node's marginal, delivered exactly symmetric.  A block with a fixed end is all zeros.
   MSFL_BAD_ARG, nothing launched or written: an index outside the nodes; a graph with no fixed node and no fix of either kind
   (structurally unanchored); free nodes but no factor.  An anchored graph can still leave a direction free (position fixes on one
   line leave the rotation about it): the factorisation's smallest pivot^2 / diagonal falls below min_pivot_ratio, the call returns
   MSFL_OK with summary.singular = 1 and every block is NaN.  Like msfl_graph_cost the call leaves poses, structure and the last
   optimize's summary and trace as they were.  The first call allocates its scratch; a graph that never asks allocates nothing. */
typedef struct msfl_graph_marginals_summary {
  int n_pairs, n_columns;          /* 6 x distinct free column nodes actually solved */
  int cg_iterations;               /* largest over the columns; 0 when the graph has no long factor (the solve is direct) */
  int cg_unconverged;              /* columns that ended at the cap; their blocks are delivered as they are */
  int singular;                    /* pivot test failed: every block is NaN */
  int pad;
  double min_pivot_ratio;          /* smallest Cholesky pivot^2 / block diagonal met in the factorisation; -1: a non-finite pivot */
} msfl_graph_marginals_summary;
typedef struct msfl_graph_marginals_options {
  double min_pivot_ratio;          /* the pivot test's threshold; default 1e-7 (anchored parity cases: 0.12 and above; gauge-free: 4e-10 and below) */
  int max_cg_iterations;           /* per column; 0: 16 x long factors + 8, as in the solve */
  int reserved;
  unsigned long long scratch_bytes;  /* budget of the column blocks (about 8 x 288 B x free nodes per column node); the column nodes
                                        are solved in chunks that fit, one at a time at the least; default 256 MiB */
} msfl_graph_marginals_options;
void        msfl_graph_marginals_default_options(msfl_graph_marginals_options* o);
msfl_status msfl_graph_marginals(msfl_graph* g, const int* pairs /* HOST, 2 x n_pairs */, int n_pairs,
                                 double* out /* 36 x n_pairs */, msfl_mem out_mem,
                                 msfl_graph_marginals_summary* summary /* may be NULL */);
msfl_status msfl_graph_marginals_with(msfl_graph* g, const int* pairs, int n_pairs, double* out, msfl_mem out_mem,
                                      const msfl_graph_marginals_options* options /* NULL: the defaults */,
                                      msfl_graph_marginals_summary* summary);
/* Covariance of T_ab = T_a^-1 T_b in the tangent of msfl_graph_edge_info (z.t + dt, z.q (x) dq(dtheta)) from the joint marginal
   [S_aa S_ab; S_ab^T S_bb] msfl_graph_marginals delivers; it can be added to a candidate closure's (L^T L)^-1.  Host arithmetic
   only.  MSFL_BAD_ARG, out untouched: a null pointer, a non-finite input or a zero quaternion. */
msfl_status msfl_graph_relative_covariance(const double pose_a[7], const double pose_b[7], const double S_aa[36],
                                           const double S_ab[36], const double S_bb[36], double out[36]);

/* ------------------------------------------------------------------------------------------------------------------
   Keyframe store: the scans themselves (their less-sharp and less-flat lists) kept on the device, and laid down at any poses
   as submaps (msfl_keyframes_compose) or into map stores (msfl_keyframes_insert).  docs/kernels/keyframes.md holds the full
   definition.  A store is created on a handle like msfl_grid, works on that handle's stream and must be destroyed before it.
   Counts are kept on the host: no call reads a size back from the device.
     add     : a list is corner[corner_idx[i]], i < n_corner (corner_idx == NULL: the array itself) - the shape of
               msfl_slam_get_clouds: full_scan with less_sharp_idx / less_flat_idx; device pointers are handed over as they are.
               With a leaf > 0 the stored list is exactly what msfl_voxel_downsample returns for the list; with leaf == 0 the
               bytes are stored unchanged.  A point with a non-finite x, y, z or t refuses the add (MSFL_BAD_ARG; host lists are
               checked before staging, device lists on the device), MSFL_CAPACITY when the keyframe count or a pool would be
               exceeded; in both cases nothing is added.  *index (optional) receives the new keyframe's index.
     sizes   : the counts of keyframes [first, first + n) into HOST arrays (either may be NULL).
     get     : one keyframe's lists (a NULL pointer: not wanted); MSFL_CAPACITY if a capacity is below the list's size.
     compose : n_submaps clouds per kind in one launch.  Submap b has the members m in [member_off[b], member_off[b + 1]); keys[m]
               and poses[7 m ..] are indexed absolutely (member_off[0] need not be 0).  Each pose [t, qx qy qz qw] maps its keyframe's
               frame into the submap's.  Per kind, C_b is the concatenation in member order of the keyframe's list transformed
               exactly as msfl_transform_cloud transforms it; the output for b is C_b (leaf == 0) or msfl_voxel_downsample(C_b, leaf).
               Outputs are written back to back, out_*_off (HOST, n_submaps + 1) starts at 0.  A key may repeat; a member without
               points contributes nothing; a submap without members is an empty cloud.  MSFL_BAD_ARG: a key that is no keyframe, a
               pose with a non-finite entry, decreasing offsets, a negative or non-finite leaf.  MSFL_CAPACITY: cap_kind below the
               sum of that kind's member counts, or that sum at 2^31 or beyond.  In every refused case nothing is launched and no
               output is written.  A transformed cloud the batch voxel filter refuses gives that call's status.  With
               MSFL_MEM_DEVICE the outputs go straight to msfl_match_pairs_batch (n_submaps == 1: msfl_set_map) and, with both
               leaves 0, the call is asynchronous.  The call uses scratch of its own: a matcher call after it is bit-identical.
     insert  : for i = 0 .. n-1 in order, keyframe keys[i] transformed by poses[7 i ..] goes through msfl_grid_insert_scan of each
               given store (either may be NULL): bit for bit the caller's loop of msfl_transform_cloud + msfl_grid_insert_scan.  The
               first keyframe a store refuses (a point beyond +-8192 cells: MSFL_CAPACITY) ends the call with that status; *n_done
               is its position, earlier keyframes stay inserted, that keyframe is in neither store.  MSFL_BAD_ARG (nothing
               inserted): a key that is no keyframe, a non-finite pose entry, a grid of another handle. */
typedef struct msfl_keyframes_s msfl_keyframes;
typedef struct msfl_keyframes_config {
  int   max_keyframes;       /* default 4096 */
  int   max_corner_points;   /* pool, fixed at creation; default 4 194 304 */
  int   max_surf_points;     /* default 16 777 216 */
  float leaf_corner;         /* voxel filter applied by add; default 0.2, 0 = store the list as given */
  float leaf_surf;           /* default 0.4, 0 = as given */
} msfl_keyframes_config;

void        msfl_keyframes_default_config(msfl_keyframes_config* c);
msfl_status msfl_keyframes_create(msfl_handle* h, const msfl_keyframes_config* c /* NULL = defaults */, msfl_keyframes** out);
void        msfl_keyframes_destroy(msfl_keyframes* k);
int         msfl_keyframes_size(const msfl_keyframes* k);
msfl_status msfl_keyframes_add(msfl_keyframes* k,
                               const msfl_point* corner, const int* corner_idx, int n_corner,
                               const msfl_point* surf,   const int* surf_idx,   int n_surf,
                               msfl_mem mem, int* index);
msfl_status msfl_keyframes_sizes(msfl_keyframes* k, int first, int n, int* n_corner, int* n_surf);   /* HOST arrays */
msfl_status msfl_keyframes_get(msfl_keyframes* k, int index, msfl_point* corner, int cap_corner,
                               msfl_point* surf, int cap_surf, msfl_mem mem);
msfl_status msfl_keyframes_compose(msfl_keyframes* k, int n_submaps,
                                   const int* member_off /* HOST, n_submaps+1 */, const int* keys /* HOST */,
                                   const double* poses /* HOST, 7 per member */,
                                   float leaf_corner, float leaf_surf,
                                   msfl_point* out_corner, int cap_corner, int* out_corner_off /* HOST, n_submaps+1 */,
                                   msfl_point* out_surf,   int cap_surf,   int* out_surf_off,
                                   msfl_mem mem);
msfl_status msfl_keyframes_insert(msfl_keyframes* k, const int* keys, const double* poses, int n,
                                  msfl_grid* grid_corner /* may be NULL */, msfl_grid* grid_surf /* may be NULL */, int* n_done);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* MSFL_C_API_H_ */
