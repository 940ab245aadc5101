"""ctypes binding of the C ABI (include/msfl_c_api.h) exported by msf_loam_amd/libmsfl_hip.so.

This is plumbing for the Python harness (tests, bench.py).  It never falls back to a CPU path:
if the shared library is missing or a call fails, it raises.
"""
import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MSFL_LIB: load another build of the same library (A/B runs of kernel variants)
LIB_PATH = os.environ.get("MSFL_LIB") or os.path.join(_HERE, "libmsfl_hip.so")

OK, TOO_FEW_CORRESPONDENCES, MAP_TOO_SMALL, BAD_ARG, HIP_ERROR, BAD_RING, NO_MAP, CAPACITY = range(8)
MEM_HOST, MEM_DEVICE = 0, 1

# One prototype per function of include/msfl_c_api.h, in the header's order: name=return:parameters.  Returns: i msfl_status / int,
# v void, z const char*.  Parameters: p any pointer or array (c_void_p), i int / msfl_mem, d double, f float.  load() applies them all;
# tests/test_capi_symbols.py holds the table against the header.  (The msfl_debug_* exports of profile builds stay undeclared.)
_CTYPE = {"i": C.c_int, "v": None, "z": C.c_char_p, "p": C.c_void_p, "d": C.c_double, "f": C.c_float}
PROTOTYPES = dict(t.split("=") for t in """
    msfl_default_params=v:p msfl_api_version=i: msfl_create=i:pip msfl_destroy=v:p msfl_set_stream=i:pp msfl_reset_stream=i:p msfl_synchronize=i:p
    msfl_status_string=z:i msfl_last_error=z:p msfl_set_timing=i:pi msfl_get_timing=i:ppi msfl_set_uncertainty=i:ppiid msfl_set_pose_prior=i:ppii
    msfl_set_degeneracy=i:pidpii msfl_set_outlier_rejection=i:pppii msfl_set_map=i:ppipii msfl_match_scan2map=i:ppipippi
    msfl_match_scan2map_batch=i:pipppppppi msfl_match_pairs_batch=i:pipppppppppppi msfl_score_poses=i:ppipipidpppi
    msfl_score_poses_batch=i:pippppppdpi msfl_set_pair_maps=i:pippppi msfl_score_pairs=i:pippppppdpppi msfl_match_pairs_resident=i:pipppppppi
    msfl_search_default_config=v:p msfl_search_geometry=i:ppiip msfl_search_poses=i:ppipipppippi msfl_relocalize=i:ppipippididpipi
    msfl_search_pairs=i:pipppppppippi
    msfl_associate_scan2map=i:ppipipp msfl_solve_records=i:ppipippp msfl_match_scan2map_deskew=i:ppipippp msfl_associate_scan2map_deskew=i:ppipipppp
    msfl_solve_records_deskew=i:ppipipppp msfl_match_scan2map_deskew_batch=i:pippppppppi msfl_match_scan2scan=i:pppppppi
    msfl_match_scan2scan_batch=i:pipppppppi msfl_extract_features=i:pppippi msfl_extract_features_batch=i:pipppppi msfl_voxel_downsample=i:ppifppi
    msfl_voxel_downsample_batch=i:pippppfppi msfl_voxel_downsample_batch_pair=i:pippppfppppfppi msfl_transform_cloud=i:ppippi msfl_delta_qp=i:pppippi
    msfl_deskew_cloud=i:pppipppi msfl_undistort_cloud=i:pppii msfl_grid_create=i:pffp msfl_grid_destroy=v:p msfl_grid_insert_scan=i:ppii
    msfl_grid_get_surrounded=i:ppippipi msfl_grid_size=i:ppp msfl_grid_dump=i:ppipi msfl_grid_dump_cells=i:ppip msfl_grid_stats=i:pp
    msfl_grid_crop=i:ppppiip msfl_grid_crop_tiles=i:ppppipiip msfl_grid_load_cells=i:ppipiipp msfl_carve_default_config=v:p msfl_carve_tables=i:ppppp
    msfl_grid_carve=i:ppipppiip msfl_grid_render=i:ppppiip msfl_novelty_default_config=v:p msfl_scan_novelty=i:ppipppppi
    msfl_grids_scan_novelty=i:pipippppppi msfl_segment_default_config=v:p msfl_segment_tables=i:pppppp msfl_segment_scans=i:pippppppppi
    msfl_segment_scan=i:pppipppppi msfl_slam_default_config=v:p msfl_slam_create=i:ppip
    msfl_slam_destroy=v:p msfl_slam_add_scan=i:pppiip msfl_slam_add_scan_imu=i:pppiipp msfl_slam_get_result=i:pip msfl_slam_set_uncertainty=i:pid
    msfl_slam_get_uncertainty=i:pipp msfl_slam_set_degeneracy=i:piidd msfl_slam_get_degeneracy=i:pipp msfl_slam_set_outlier_rejection=i:ppp
    msfl_slam_get_rejection=i:pipp msfl_slam_set_next_prior=i:ppp msfl_slam_set_map_window=i:ppi msfl_slam_get_map_window=i:pipp
    msfl_slam_get_clouds=i:pipi msfl_slam_grids=i:ppp msfl_slam_last_error=z:p msfl_places_default_config=v:p msfl_places_create=i:pip
    msfl_places_destroy=v:p msfl_places_set_stream=i:pp msfl_places_synchronize=i:p msfl_places_size=i:p msfl_places_last_error=z:p
    msfl_places_add=i:pppiip msfl_places_add_descriptors=i:ppiip msfl_places_get=i:piippi msfl_places_query=i:pppipiipi
    msfl_places_query_entries=i:ppipiipi msfl_graph_default_config=v:p msfl_graph_create=i:pip msfl_graph_destroy=v:p msfl_graph_set_stream=i:pp
    msfl_graph_synchronize=i:p msfl_graph_last_error=z:p msfl_graph_clear=i:p msfl_graph_num_nodes=i:p msfl_graph_add_nodes=i:ppiip
    msfl_graph_add_edges=i:ppi msfl_graph_add_fixes=i:ppi msfl_graph_set_fixed=i:pii msfl_graph_set_poses=i:piipi msfl_graph_get_poses=i:piipi
    msfl_graph_cost=i:pp msfl_graph_optimize=i:pp msfl_graph_get_trace=i:pppip msfl_graph_add_edges_info=i:ppi msfl_graph_add_fixes_info=i:ppi
    msfl_graph_edge_from_uncertainty=i:iipppdp msfl_graph_fix_from_covariance=i:iidppp msfl_graph_factor_chi2=i:piiip msfl_graph_set_losses=i:piiipi
    msfl_graph_get_losses=i:piiip msfl_graph_factor_weights=i:piiip msfl_graph_marginals_default_options=v:p msfl_graph_marginals=i:ppipip
    msfl_graph_marginals_with=i:ppipipp msfl_graph_relative_covariance=i:pppppp msfl_keyframes_default_config=v:p msfl_keyframes_create=i:ppp
    msfl_keyframes_destroy=v:p msfl_keyframes_size=i:p msfl_keyframes_add=i:pppippiip msfl_keyframes_sizes=i:piipp msfl_keyframes_get=i:pipipii
    msfl_keyframes_compose=i:pipppffpippipi msfl_keyframes_insert=i:pppippp
""".split())
EXPORTED = list(PROTOTYPES)


class Preintegration(C.Structure):
    _fields_ = [("sum_dt", C.POINTER(C.c_double)), ("delta_q", C.POINTER(C.c_double)), ("delta_p", C.POINTER(C.c_double)),
                ("n", C.c_int)]


class Params(C.Structure):
    _fields_ = [
        ("scan_period", C.c_double), ("min_range", C.c_double),
        ("curvature_threshold", C.c_float), ("neighbor_gap_sq", C.c_float),
        ("sectors_per_ring", C.c_int), ("max_sharp_per_sector", C.c_int),
        ("max_less_sharp_per_sector", C.c_int), ("max_flat_per_sector", C.c_int),
        ("odom_distance_sq_threshold", C.c_double), ("odom_nearby_scan", C.c_double),
        ("odom_min_correspondences", C.c_int),
        ("map_knn", C.c_int), ("map_knn_max_sq_dist", C.c_float),
        ("line_eigen_ratio", C.c_double), ("plane_tolerance", C.c_double),
        ("outer_iterations", C.c_int), ("max_lm_iterations", C.c_int), ("huber_delta", C.c_double),
        ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double),
        ("min_trust_region_radius", C.c_double), ("min_relative_decrease", C.c_double),
        ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
        ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double), ("max_consecutive_invalid_steps", C.c_int),
    ]


class MatchInfo(C.Structure):
    _fields_ = [("status", C.c_int), ("n_edge", C.c_int * 2), ("n_plane", C.c_int * 2),
                ("lm_iterations", C.c_int * 2), ("lm_successful", C.c_int * 2),
                ("initial_cost", C.c_double * 2), ("final_cost", C.c_double * 2)]


class MatchUncertainty(C.Structure):
    """msfl_match_uncertainty: information matrix of the last solve at the returned pose, its eigen-decomposition and covariance."""
    _fields_ = [("information", C.c_double * 36), ("eigenvalues", C.c_double * 6), ("eigenvectors", C.c_double * 36),
                ("covariance", C.c_double * 36), ("sigma2", C.c_double), ("n_residuals", C.c_int), ("n_degenerate", C.c_int),
                ("valid", C.c_int), ("reserved_", C.c_int)]


# the same record as a numpy structured dtype (Handle.uncertainty, Slam.get_uncertainty)
UNCERTAINTY_DTYPE = np.dtype([("information", np.float64, (6, 6)), ("eigenvalues", np.float64, (6,)), ("eigenvectors", np.float64, (6, 6)),
                              ("covariance", np.float64, (6, 6)), ("sigma2", np.float64), ("n_residuals", np.int32),
                              ("n_degenerate", np.int32), ("valid", np.int32), ("reserved_", np.int32)])
assert UNCERTAINTY_DTYPE.itemsize == C.sizeof(MatchUncertainty)


class PosePrior(C.Structure):
    """msfl_pose_prior: prior mean (t0, q0 xyzw) and the row-major 6 x 6 square-root information L (information = L^T L)."""
    _fields_ = [("pose", C.c_double * 7), ("sqrt_information", C.c_double * 36)]


# the same record as a numpy structured dtype (Handle.set_pose_prior, Slam.set_next_prior)
POSE_PRIOR_DTYPE = np.dtype([("pose", np.float64, (7,)), ("sqrt_information", np.float64, (6, 6))])
assert POSE_PRIOR_DTYPE.itemsize == C.sizeof(PosePrior)


class DegeneracyRecord(C.Structure):
    """msfl_degeneracy_record: per outer iteration the eigen-decomposition of the solve's entry matrix and the number of held directions."""
    _fields_ = [("eigenvalues", (C.c_double * 6) * 2), ("eigenvectors", (C.c_double * 36) * 2), ("n_held", C.c_int * 2), ("valid", C.c_int * 2)]


# the same record as a numpy structured dtype (Handle.degeneracy, Slam.get_degeneracy)
DEGENERACY_DTYPE = np.dtype([("eigenvalues", np.float64, (2, 6)), ("eigenvectors", np.float64, (2, 6, 6)), ("n_held", np.int32, (2,)),
                             ("valid", np.int32, (2,))])
assert DEGENERACY_DTYPE.itemsize == C.sizeof(DegeneracyRecord) == 688


REJECT_OFF, REJECT_THRESHOLD, REJECT_FRACTION = 0, 1, 2          # msfl_outlier_rejection.mode
REJECT_LAST_OUTER, REJECT_EVERY_OUTER = 0, 1                      # msfl_outlier_rejection.which


class OutlierRejection(C.Structure):
    """msfl_outlier_rejection: mode, threshold (THRESHOLD), fraction (FRACTION) and the solves it runs in front of."""
    _fields_ = [("mode", C.c_int), ("threshold", C.c_double), ("fraction", C.c_double), ("which", C.c_int)]


class RejectionRecord(C.Structure):
    """msfl_rejection_record: per outer iteration the correspondences entering the solve, those rejected and the cut."""
    _fields_ = [("n_edge_in", C.c_int * 2), ("n_plane_in", C.c_int * 2), ("n_edge_rejected", C.c_int * 2), ("n_plane_rejected", C.c_int * 2),
                ("cut_sq", C.c_double * 2), ("valid", C.c_int * 2)]


# the same record as a numpy structured dtype (Handle.rejection, Slam.get_rejection)
REJECTION_DTYPE = np.dtype([("n_edge_in", np.int32, (2,)), ("n_plane_in", np.int32, (2,)), ("n_edge_rejected", np.int32, (2,)),
                            ("n_plane_rejected", np.int32, (2,)), ("cut_sq", np.float64, (2,)), ("valid", np.int32, (2,))])
assert REJECTION_DTYPE.itemsize == C.sizeof(RejectionRecord) == 56


def outlier_rejection(threshold=None, fraction=None, which=REJECT_LAST_OUTER):
    """The msfl_outlier_rejection of exactly one of `threshold` (metres) and `fraction` (of a scan's correspondences)."""
    if (threshold is None) == (fraction is None):
        raise ValueError("give exactly one of threshold and fraction")
    if threshold is not None:
        return OutlierRejection(REJECT_THRESHOLD, float(threshold), 0.0, int(which))
    return OutlierRejection(REJECT_FRACTION, 0.0, float(fraction), int(which))


class PoseScore(C.Structure):
    """msfl_pose_score: per feature kind (corner, surf) the inliers of one pose and the fixed-point sum of their squared distances."""
    _fields_ = [("inliers", C.c_int * 2), ("sum_sq_q32", C.c_ulonglong * 2), ("status", C.c_int), ("reserved_", C.c_int)]


# the same record as a numpy structured dtype (Handle.score_poses, Handle.score_poses_batch)
POSE_SCORE_DTYPE = np.dtype([("inliers", np.int32, (2,)), ("sum_sq_q32", np.uint64, (2,)), ("status", np.int32), ("reserved_", np.int32)])
assert POSE_SCORE_DTYPE.itemsize == C.sizeof(PoseScore) == 32


def fitness(scores, n_corner, n_surf):
    """Inlier fraction of each record: (corner + surf inliers) / (n_corner + n_surf); n_corner / n_surf may be per-record arrays.
    A scan without features has fitness 0."""
    n = np.asarray(n_corner, np.float64) + np.asarray(n_surf, np.float64)
    inl = scores["inliers"].sum(-1).astype(np.float64)
    return np.divide(inl, n, out=np.zeros(np.broadcast(inl, n).shape), where=n > 0)


def rmse(scores):
    """Root mean squared inlier distance of each record in metres: sqrt(sum_sq_q32 / 2^32 / inliers); NaN without inliers."""
    inl = scores["inliers"].sum(-1).astype(np.float64)
    tot = scores["sum_sq_q32"].astype(np.float64).sum(-1) / 4294967296.0     # (each sum is below 2^63; the float64 rounding is 2^-53 relative)
    return np.sqrt(np.divide(tot, inl, out=np.full(np.shape(inl), np.nan), where=inl > 0))


class SearchConfig(C.Structure):
    """msfl_search_config: the yaw x position lattice, the voxel pitch and the peak windows of Handle.search_poses.  Built with the
    library's defaults (msfl_search_default_config); keywords override fields (half: three ints)."""
    _fields_ = [("step", C.c_double), ("half", C.c_int * 3), ("n_yaw", C.c_int), ("yaw_min", C.c_double), ("yaw_step", C.c_double),
                ("yaw_wraps", C.c_int), ("dilate", C.c_int), ("range", C.c_double), ("nms_cells", C.c_int), ("nms_yaws", C.c_int),
                ("max_volume_bytes", C.c_longlong)]

    def __init__(self, **kw):
        super().__init__()
        load().msfl_search_default_config(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("SearchConfig has no field " + k)
            setattr(self, k, (C.c_int * 3)(*[int(x) for x in v]) if k == "half" else v)


class SearchGeom(C.Structure):
    """msfl_search_geom: the box, the lattice and the scratch of one search (capi.search_geometry)."""
    _fields_ = [("origin", C.c_float * 3), ("inv_step", C.c_float), ("dims", C.c_int * 3), ("words_per_row", C.c_int), ("n", C.c_int * 3),
                ("n_yaw", C.c_int), ("n_hypotheses", C.c_longlong), ("volume_bytes", C.c_longlong), ("scratch_bytes", C.c_longlong)]


POSE_CANDIDATE_DTYPE = np.dtype([("pose", np.float64, (7,)), ("h", np.int32), ("a", np.int32), ("kx", np.int32), ("ky", np.int32),
                                 ("kz", np.int32), ("hits", np.int32, (2,)), ("reserved_", np.int32)])
RELOC_RESULT_DTYPE = np.dtype([("pose", np.float64, (7,)), ("candidate", POSE_CANDIDATE_DTYPE), ("coarse", POSE_SCORE_DTYPE),
                               ("refined", POSE_SCORE_DTYPE), ("status", np.int32), ("accepted", np.int32)])
assert POSE_CANDIDATE_DTYPE.itemsize == 88 and RELOC_RESULT_DTYPE.itemsize == 216 and C.sizeof(SearchConfig) == 72


def search_geometry(guess, config, n_corner=0, n_surf=0, allow=()):
    """msfl_search_geometry, on the host alone (no handle, no GPU): (status, SearchGeom).  A status outside `allow` raises."""
    guess = np.ascontiguousarray(np.asarray(guess, np.float64).reshape(7))
    g = SearchGeom()
    s = load().msfl_search_geometry(_vp(guess), C.byref(config), int(n_corner), int(n_surf), C.byref(g))
    if s != OK and s not in allow:
        raise MsflError(s, "msfl_search_geometry")
    return s, g


class PlaceConfig(C.Structure):
    """msfl_place_config: polar bins, range gate, height offset and the fixed capacity of the database."""
    _fields_ = [("n_ring", C.c_int), ("n_sector", C.c_int), ("min_range", C.c_double), ("max_range", C.c_double),
                ("height_offset", C.c_double), ("capacity", C.c_int)]


class PlaceMatch(C.Structure):
    """msfl_place_match: one candidate of a query, its column shift and its rotation-invariant distance."""
    _fields_ = [("index", C.c_int), ("shift", C.c_int), ("ring_key_d2", C.c_int), ("n_columns", C.c_int), ("distance", C.c_double)]


# the same record as a numpy structured dtype (Places.query, Places.query_entries)
PLACE_MATCH_DTYPE = np.dtype([("index", np.int32), ("shift", np.int32), ("ring_key_d2", np.int32), ("n_columns", np.int32),
                              ("distance", np.float64)])
assert PLACE_MATCH_DTYPE.itemsize == C.sizeof(PlaceMatch) == 24


def place_yaw(shift, n_sector):
    """Yaw in radians, in (-pi, pi], that a column shift stands for (steps of 2 pi / n_sector); arrays welcome."""
    a = 2.0 * np.pi * (np.asarray(shift) % int(n_sector)) / int(n_sector)
    return np.where(a > np.pi, a - 2.0 * np.pi, a)[()]


def _on_device(x):
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def pose_priors(poses, sqrt_info):
    """(B, 7) prior means and (B, 6, 6) square-root information matrices -> B records of POSE_PRIOR_DTYPE."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 7)
    rec = np.zeros(len(poses), POSE_PRIOR_DTYPE)
    rec["pose"] = poses
    rec["sqrt_information"] = np.asarray(sqrt_info, dtype=np.float64).reshape(len(poses), 6, 6)
    return rec


class Timing(C.Structure):
    _fields_ = [("launches_assoc", C.c_int), ("ms_assoc", C.c_double),
                ("launches_solve", C.c_int), ("ms_solve", C.c_double),
                ("launches_index", C.c_int), ("ms_index", C.c_double),
                ("launches_extract", C.c_int), ("ms_extract", C.c_double),
                ("launches_odom", C.c_int), ("ms_odom", C.c_double),
                ("launches_fit", C.c_int), ("ms_fit", C.c_double), ("knn_candidates", C.c_ulonglong), ("knn_candidates_seeded", C.c_ulonglong),
                ("launches_assoc_seeded", C.c_int), ("ms_assoc_seeded", C.c_double)]


class Deskew(C.Structure):
    _fields_ = [("corner_dq", C.c_void_p), ("corner_dp", C.c_void_p), ("surf_dq", C.c_void_p),
                ("surf_dp", C.c_void_p), ("velocity", C.c_double * 3), ("gravity", C.c_double * 3)]


class DeskewBatch(C.Structure):
    _fields_ = [("corner_dq", C.c_void_p), ("corner_dp", C.c_void_p), ("surf_dq", C.c_void_p),
                ("surf_dp", C.c_void_p), ("velocity", C.c_void_p), ("gravity", C.c_double * 3)]


class RingCloud(C.Structure):
    _fields_ = [("pts", C.c_void_p), ("ring", C.c_void_p), ("n", C.c_int)]


class RingCloudBatch(C.Structure):
    _fields_ = [("pts", C.c_void_p), ("ring", C.c_void_p), ("off", C.c_void_p)]


class Features(C.Structure):
    _fields_ = [("full_pts", C.c_void_p), ("full_ring", C.c_void_p), ("curvature", C.c_void_p),
                ("label", C.c_void_p), ("sharp_idx", C.c_void_p), ("less_sharp_idx", C.c_void_p),
                ("flat_idx", C.c_void_p), ("less_flat_idx", C.c_void_p),
                ("n_full", C.c_int), ("n_sharp", C.c_int), ("n_less_sharp", C.c_int),
                ("n_flat", C.c_int), ("n_less_flat", C.c_int)]


class FeaturesBatch(C.Structure):
    _fields_ = [("full_pts", C.c_void_p), ("full_ring", C.c_void_p), ("curvature", C.c_void_p),
                ("label", C.c_void_p), ("sharp_idx", C.c_void_p), ("less_sharp_idx", C.c_void_p),
                ("flat_idx", C.c_void_p), ("less_flat_idx", C.c_void_p),
                ("n_full", C.c_void_p), ("n_sharp", C.c_void_p), ("n_less_sharp", C.c_void_p),
                ("n_flat", C.c_void_p), ("n_less_flat", C.c_void_p)]


class GridCropInfo(C.Structure):
    """msfl_grid_crop_info; `status` (a Python attribute) is the msfl_status of the call that filled it."""
    _fields_ = [("n_cells_evicted", C.c_int), ("n_points_evicted", C.c_int), ("n_cells", C.c_int), ("n_points", C.c_int),
                ("center_cell", C.c_int * 3), ("applied", C.c_int)]
    status = OK

    def as_tuple(self):
        return (self.n_cells_evicted, self.n_points_evicted, self.n_cells, self.n_points, tuple(self.center_cell), self.applied)


class GridLoadInfo(C.Structure):
    """msfl_grid_load_info; `status` (a Python attribute) is the msfl_status of the call that filled it."""
    _fields_ = [("n_cells_loaded", C.c_int), ("n_points_loaded", C.c_int), ("n_cells", C.c_int), ("n_points", C.c_int),
                ("n_conflicts", C.c_int), ("n_bad_points", C.c_int), ("applied", C.c_int), ("reserved_", C.c_int)]
    status = OK

    def as_tuple(self):
        return (self.n_cells_loaded, self.n_points_loaded, self.n_cells, self.n_points, self.n_conflicts, self.n_bad_points, self.applied)


class CarveConfig(C.Structure):
    """msfl_carve_config (include/msfl_c_api.h, "Carve")."""
    _fields_ = [("n_col", C.c_int), ("n_row", C.c_int), ("elev_low_deg", C.c_float), ("elev_high_deg", C.c_float),
                ("min_range", C.c_float), ("max_range", C.c_float), ("margin_abs", C.c_float), ("margin_rel", C.c_float),
                ("window_col", C.c_int), ("window_row", C.c_int)]


def carve_config(**kw):
    """msfl_carve_default_config with the given fields replaced."""
    c = CarveConfig()
    load().msfl_carve_default_config(C.byref(c))
    for k, v in kw.items():
        if k not in dict(CarveConfig._fields_):
            raise TypeError("msfl_carve_config has no field " + k)
        setattr(c, k, v)
    return c


def carve_tables(config=None):
    """msfl_carve_tables: (cc, cs, ec, es) as f32 arrays, the tables msfl_grid_carve bisects over (a pure host call)."""
    c = config if config is not None else carve_config()
    cc, cs = np.zeros(max(c.n_col // 2, 1), np.float32), np.zeros(max(c.n_col // 2, 1), np.float32)
    ec, es = np.zeros(max(c.n_row + 1, 1), np.float32), np.zeros(max(c.n_row + 1, 1), np.float32)
    s = load().msfl_carve_tables(C.byref(c), _vp(cc), _vp(cs), _vp(ec), _vp(es))
    if s != OK:
        raise MsflError(s, "msfl_carve_tables")
    return cc, cs, ec, es


class GridCarveInfo(C.Structure):
    """msfl_grid_carve_info; `status` (a Python attribute) is the msfl_status of the call that filled it."""
    _fields_ = [("n_points_removed", C.c_int), ("n_cells_emptied", C.c_int), ("n_cells", C.c_int), ("n_points", C.c_int),
                ("n_tested", C.c_int), ("n_pixels", C.c_int), ("applied", C.c_int), ("reserved_", C.c_int)]
    status = OK

    def as_tuple(self):
        return (self.n_points_removed, self.n_cells_emptied, self.n_cells, self.n_points, self.n_tested, self.n_pixels, self.applied)


NOV_NONE, NOV_UNSEEN, NOV_COVERED, NOV_IN_FRONT = range(4)                   # MSFL_NOV_*: the classes of msfl_scan_novelty
NOV_CLASS_NAMES = ("none", "unseen", "covered", "in_front")


class GridRenderInfo(C.Structure):
    """msfl_grid_render_info; `status` (a Python attribute) is the msfl_status of the call that filled it."""
    _fields_ = [("n_tested", C.c_int), ("applied", C.c_int)]
    status = OK


class NoveltyConfig(C.Structure):
    """msfl_novelty_config (include/msfl_c_api.h, docs/kernels/novelty.md): `image` is a CarveConfig."""
    _fields_ = [("image", CarveConfig), ("min_support", C.c_int), ("keep_classes", C.c_int)]


def novelty_config(**kw):
    """msfl_novelty_default_config with the given fields replaced; a field of msfl_carve_config goes into `image`."""
    c = NoveltyConfig()
    load().msfl_novelty_default_config(C.byref(c))
    for k, v in kw.items():
        if k in ("min_support", "keep_classes"):
            setattr(c, k, v)
        elif k in dict(CarveConfig._fields_):
            setattr(c.image, k, v)
        else:
            raise TypeError("msfl_novelty_config has no field " + k)
    return c


class NoveltyInfo(C.Structure):
    """msfl_novelty_info; `status` (a Python attribute) is the msfl_status of the call that filled it."""
    _fields_ = [("n_class", C.c_int * 4), ("n_map_pixels", C.c_int), ("n_kept", C.c_int), ("applied", C.c_int), ("reserved_", C.c_int)]
    status = OK

    def as_tuple(self):
        return (tuple(self.n_class), self.n_map_pixels, self.n_kept, self.applied)


def _novelty_host(call, scan, config, want_masked, what, check, allow):
    """The host-memory half shared by Handle.scan_novelty and grids_scan_novelty: call(scan, n, cfg, cls, masked, info) is the C
    call with its other arguments bound.  Returns dict(cls, masked, info)."""
    scan = _pts(scan)
    n = len(scan)
    cls = np.zeros(max(n, 1), np.uint8)
    masked = np.zeros((max(n, 1), 4), np.float32) if want_masked else None
    info = NoveltyInfo()
    cfg = C.byref(config) if config is not None else None
    info.status = check(call(_vp(scan), n, cfg, _vp(cls), _vp(masked), C.byref(info)), what, allow)
    return dict(cls=cls[:n], masked=None if masked is None else masked[:n], info=info)


def grids_scan_novelty(grids, scan, pose, config=None, want_masked=True, want_image=False, allow=()):
    """msfl_grids_scan_novelty through host memory: render `grids` (Grid objects of one handle) at the map pose `pose` into one image
    and label `scan` (sensor frame) against it.  Returns dict(cls, masked, info, image): cls uint8 per point (NOV_*), masked the
    cloud with the dropped points set to NaN, info a NoveltyInfo, image (n_row, n_col) f32 with want_image."""
    grids = list(grids)
    cfg = config if config is not None else novelty_config()
    arr = (C.c_void_p * max(len(grids), 1))(*[g.g.value for g in grids])
    pose = np.ascontiguousarray(pose, dtype=np.float64)
    img = np.zeros((cfg.image.n_row, cfg.image.n_col), np.float32) if want_image else None
    lib, owner = grids[0].lib, grids[0]
    out = _novelty_host(lambda s, n, c, cls, m, info: lib.msfl_grids_scan_novelty(arr, len(grids), s, n, _vp(pose), c, cls, m, _vp(img), info, MEM_HOST),
                        scan, cfg, want_masked, "msfl_grids_scan_novelty", owner._check, allow)
    out["image"] = img
    return out


def grids_scan_novelty_device(grids, scan_ptr, n, pose_ptr, config, cls_ptr, masked_ptr=None, image_ptr=None, want_info=False, allow=()):
    """msfl_grids_scan_novelty with the scan, the pose (7 doubles) and the outputs in device memory.  Without want_info the call
    only enqueues and returns None; with it the NoveltyInfo."""
    grids = list(grids)
    arr = (C.c_void_p * max(len(grids), 1))(*[g.g.value for g in grids])
    info = NoveltyInfo() if want_info else None
    cfg = C.byref(config) if config is not None else None
    s = grids[0]._check(grids[0].lib.msfl_grids_scan_novelty(arr, len(grids), _vp(scan_ptr), int(n), _vp(pose_ptr), cfg, _vp(cls_ptr), _vp(masked_ptr),
                                                             _vp(image_ptr), C.byref(info) if want_info else None, MEM_DEVICE),
                        "msfl_grids_scan_novelty(device)", allow)
    if want_info:
        info.status = s
    return info


SEG_NONE, SEG_SHADOWED, SEG_GROUND, SEG_SEGMENT, SEG_OUTLIER = range(5)      # MSFL_SEG_*: the classes of msfl_segment_scans
SEG_CLASS_NAMES = ("none", "shadowed", "ground", "segment", "outlier")


class SegmentConfig(C.Structure):
    """msfl_segment_config (include/msfl_c_api.h, docs/kernels/segment.md), built with the library's defaults
    (msfl_segment_default_config); keywords override fields.  up: three floats; row_elev_deg: None or n_row ascending elevations
    (the array is kept alive by this object)."""
    _fields_ = [("n_col", C.c_int), ("n_row", C.c_int), ("elev_low_deg", C.c_float), ("elev_high_deg", C.c_float),
                ("row_elev_deg", C.c_void_p), ("min_range", C.c_float), ("max_range", C.c_float), ("ground_rows", C.c_int),
                ("ground_angle_deg", C.c_float), ("up", C.c_float * 3), ("segment_angle_deg", C.c_float), ("min_points", C.c_int),
                ("min_points_tall", C.c_int), ("min_rows_tall", C.c_int), ("keep_classes", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        load().msfl_segment_default_config(C.byref(self))
        self._rows = None
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("SegmentConfig has no field " + k)
            if k == "row_elev_deg":
                self._rows = None if v is None else np.ascontiguousarray(v, dtype=np.float32)
                v = None if v is None else self._rows.ctypes.data
            elif k == "up":
                v = (C.c_float * 3)(*[float(x) for x in v])
            setattr(self, k, v)


SEGMENT_INFO_DTYPE = np.dtype([("n_class", np.int32, (5,)), ("n_pixels", np.int32), ("n_components", np.int32), ("n_segments", np.int32),
                               ("n_kept", np.int32), ("reserved_", np.int32)])
assert SEGMENT_INFO_DTYPE.itemsize == 40 and C.sizeof(SegmentConfig) == 72


def segment_tables(config=None):
    """msfl_segment_tables: (cc, cs, vs, vc, scalars) as f32 arrays, the tables msfl_segment_scans compares against (a pure host
    call).  scalars = [sin, cos of one column, sin^2(ground angle), tan(segment angle)]."""
    c = config if config is not None else SegmentConfig()
    cc, cs = np.zeros(max(c.n_col // 2, 1), np.float32), np.zeros(max(c.n_col // 2, 1), np.float32)
    vs, vc = np.zeros(max(c.n_row - 1, 1), np.float32), np.zeros(max(c.n_row - 1, 1), np.float32)
    scalars = np.zeros(4, np.float32)
    s = load().msfl_segment_tables(C.byref(c), _vp(cc), _vp(cs), _vp(vs), _vp(vc), _vp(scalars))
    if s != OK:
        raise MsflError(s, "msfl_segment_tables")
    return cc, cs, vs, vc, scalars


GRID_STATS = ("n_points", "n_cells", "pool_top", "pool_capacity_points", "cell_capacity", "device_bytes")


class SlamConfig(C.Structure):
    _fields_ = [("map_resolution", C.c_float), ("leaf_corner", C.c_float), ("leaf_surf", C.c_float),
                ("min_map_corner", C.c_int), ("min_map_surf", C.c_int), ("max_scan_points", C.c_int), ("max_rings", C.c_int),
                ("pose_odom2map", C.c_double * 7), ("reference_quirks", C.c_int), ("keep_clouds", C.c_int)]


class SlamClouds(C.Structure):
    """msfl_slam_clouds: cloud_full_res after the IMU passes, its map-frame copy, ring ids and the four index lists (keep_clouds)."""
    _fields_ = [("full_scan", C.c_void_p), ("full_map", C.c_void_p), ("ring", C.c_void_p),
                ("sharp_idx", C.c_void_p), ("less_sharp_idx", C.c_void_p), ("flat_idx", C.c_void_p), ("less_flat_idx", C.c_void_p),
                ("n_full", C.c_int), ("n_sharp", C.c_int), ("n_less_sharp", C.c_int), ("n_flat", C.c_int), ("n_less_flat", C.c_int)]


class SlamImu(C.Structure):
    """msfl_slam_imu: the per-scan IMU inputs of LaserMapping::Run (laser_mapping.cc:170-176,197-211)."""
    _fields_ = [("pre", C.POINTER(Preintegration)), ("is_initialized", C.c_int), ("velocity", C.c_double * 3),
                ("gravity", C.c_double * 3), ("presolved_pose", C.c_double * 7)]


class SlamResult(C.Structure):
    _fields_ = [("pose_odom", C.c_double * 7), ("pose_map", C.c_double * 7), ("pose_curr2last", C.c_double * 7),
                ("pose_odom2map", C.c_double * 7), ("odometry", MatchInfo), ("mapping", MatchInfo),
                ("scan_index", C.c_int), ("status_extract", C.c_int), ("status_mapping", C.c_int),
                ("n_full", C.c_int), ("n_sharp", C.c_int), ("n_less_sharp", C.c_int), ("n_flat", C.c_int), ("n_less_flat", C.c_int),
                ("n_corner_ds", C.c_int), ("n_surf_ds", C.c_int), ("n_map_corner", C.c_int), ("n_map_surf", C.c_int),
                ("grid_corner", C.c_int * 8), ("grid_surf", C.c_int * 8), ("status_imu", C.c_int), ("status_insert", C.c_int),
                ("status_clouds", C.c_int), ("reserved_", C.c_int)]


class MsflError(RuntimeError):
    def __init__(self, status, what, detail=""):
        self.status = status
        super().__init__(f"{what}: status {status} ({status_string(status)}) {detail}")


_lib = None


def load():
    """Load libmsfl_hip.so.  Raises (never falls back) if the HIP extension is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, sig in PROTOTYPES.items():                        # a missing export raises here, by name
            ret, params = sig.split(":")
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = _CTYPE[ret], [_CTYPE[k] for k in params]
        _lib = lib
    return _lib


def status_string(s):
    return load().msfl_status_string(int(s)).decode()


def default_params():
    p = Params()
    load().msfl_default_params(C.byref(p))
    return p


def _vp(x):
    """numpy array / int device pointer / torch tensor / None -> c_void_p"""
    if x is None:
        return C.c_void_p(None)
    if isinstance(x, int):
        return C.c_void_p(x)
    if isinstance(x, np.ndarray):
        return C.c_void_p(x.ctypes.data)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    raise TypeError(type(x))


def _pts(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 4))


class _Owner:
    """What the six owners share: `lib`, one opaque pointer (the attribute _PTR names), the function that destroys it and the one
    that delivers its error text (_ERROR None: the text is the parent handle's)."""
    _PTR = _DESTROY = _ERROR = None
    _dependents = ()                                                # objects to close before this one (Handle)

    def _own(self, lib):
        """Starts with a null pointer; returns the reference msfl_*_create fills."""
        self.lib = lib
        setattr(self, self._PTR, C.c_void_p())
        return C.byref(getattr(self, self._PTR))

    def close(self):
        p = getattr(self, self._PTR)
        if p:
            for d in list(self._dependents):                        # a grid must be destroyed before its handle (msfl_c_api.h)
                d.close()
            getattr(self.lib, self._DESTROY)(p)
            setattr(self, self._PTR, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        if self._ERROR is None:
            return self.handle.last_error()
        return (getattr(self.lib, self._ERROR)(getattr(self, self._PTR)) or b"").decode()

    def _check(self, status, what, allow=()):
        if status != OK and status not in allow:
            raise MsflError(status, what, self.last_error())
        return status


class Handle(_Owner):
    """Owns one msfl_handle (one HIP stream + device scratch)."""
    _PTR, _DESTROY, _ERROR = "h", "msfl_destroy", "msfl_last_error"
    # the record sinks: attribute of the host buffer, its dtype, what reading says when there is none
    _SINKS = {"uncertainty": ("_unc", UNCERTAINTY_DTYPE, "uncertainty output is off: call set_uncertainty(n) first"),
              "degeneracy": ("_degen", DEGENERACY_DTYPE, "no degeneracy record sink: call set_degeneracy(min_eigenvalue, n) first"),
              "rejection": ("_reject", REJECTION_DTYPE, "no rejection record sink: call set_outlier_rejection(..., n=n) first")}

    def __init__(self, device=0, params=None):
        self._dependents = weakref.WeakSet()                        # the open Grid / Keyframes objects on this handle
        self._unc = self._degen = self._reject = self._prior = None
        ref = self._own(load())
        s = self.lib.msfl_create(C.byref(params) if params is not None else None, device, ref)
        if s != OK:
            raise MsflError(s, "msfl_create", "(no GPU / HIP runtime? there is no CPU fallback)")

    def _set_sink(self, kind, call, what, ptr=None, capacity=0, mem=MEM_HOST):
        """Points one record sink somewhere: call(ptr, capacity, mem) is the msfl_set_* call with its other arguments bound.  Host
        memory with a capacity: a fresh structured array that this object keeps (what _records reads); a device pointer or no sink
        drops it.  The old array goes only once the library has taken the new sink."""
        capacity = int(capacity or 0)
        buf = np.zeros(capacity, self._SINKS[kind][1]) if mem == MEM_HOST and capacity else None
        self._check(call(_vp(ptr if buf is None else buf), capacity, mem), what)
        setattr(self, self._SINKS[kind][0], buf)

    def _records(self, kind, n):
        """The first `n` records (default: all) the last matcher call wrote into the kept host sink, as a copy."""
        attr, _, missing = self._SINKS[kind]
        buf = getattr(self, attr)
        if buf is None:
            raise RuntimeError(missing)
        return buf[:len(buf) if n is None else int(n)].copy()

    # ---- plumbing ----
    def set_stream(self, stream_ptr):
        self._check(self.lib.msfl_set_stream(self.h, stream_ptr), "msfl_set_stream")

    def reset_stream(self):
        self._check(self.lib.msfl_reset_stream(self.h), "msfl_reset_stream")

    def synchronize(self):
        self._check(self.lib.msfl_synchronize(self.h), "msfl_synchronize")

    def set_timing(self, on=True):
        self._check(self.lib.msfl_set_timing(self.h, int(on)), "msfl_set_timing")

    def get_timing(self, reset=True):
        t = Timing()
        self._check(self.lib.msfl_get_timing(self.h, C.byref(t), int(reset)), "msfl_get_timing")
        return t

    # ---- uncertainty output (msfl_set_uncertainty) ----
    def set_uncertainty(self, n, min_eigenvalue=0.0):
        """Every later matcher call writes one msfl_match_uncertainty per registration into a host buffer of `n` records
        owned by this object (read it with uncertainty()).  n = 0 / None turns the feature off."""
        eig = min_eigenvalue if n else 0.0
        self._set_sink("uncertainty", lambda p, cap, mem: self.lib.msfl_set_uncertainty(self.h, p, cap, mem, eig), "msfl_set_uncertainty",
                       capacity=n)

    def uncertainty(self, n=None):
        """The first `n` records (default: all) the last matcher call wrote, as a copy of the numpy structured array."""
        return self._records("uncertainty", n)

    def set_uncertainty_device(self, ptr, capacity, min_eigenvalue=0.0):
        """Device-pointer variant for the *_device calls: `ptr` (torch tensor / raw pointer / None = off) holds `capacity` records of
        UNCERTAINTY_DTYPE.itemsize bytes; written asynchronously on the handle's stream."""
        self._set_sink("uncertainty", lambda p, cap, mem: self.lib.msfl_set_uncertainty(self.h, p, cap, mem, min_eigenvalue),
                       "msfl_set_uncertainty(device)", ptr, capacity if ptr is not None else 0, MEM_DEVICE)

    # ---- degeneracy-aware solve (msfl_set_degeneracy) ----
    def set_degeneracy(self, min_eigenvalue, n=0):
        """Every later solve holds the eigen-directions of its entry matrix below `min_eigenvalue` at the guess.  n > 0: one
        msfl_degeneracy_record per registration goes to a host buffer of `n` records owned by this object (read it with degeneracy())."""
        self._set_sink("degeneracy", lambda p, cap, mem: self.lib.msfl_set_degeneracy(self.h, 1, min_eigenvalue, p, cap, mem),
                       "msfl_set_degeneracy", capacity=n)

    def set_degeneracy_device(self, min_eigenvalue, ptr, capacity):
        """Device-pointer sink: `ptr` (torch tensor / raw pointer) holds `capacity` records of DEGENERACY_DTYPE.itemsize bytes, written
        asynchronously on the handle's stream."""
        self._set_sink("degeneracy", lambda p, cap, mem: self.lib.msfl_set_degeneracy(self.h, 1, min_eigenvalue, p, cap, mem),
                       "msfl_set_degeneracy(device)", ptr, capacity, MEM_DEVICE)

    def clear_degeneracy(self):
        self._set_sink("degeneracy", lambda p, cap, mem: self.lib.msfl_set_degeneracy(self.h, 0, 0.0, p, cap, mem), "msfl_set_degeneracy")

    # ---- outlier rejection in front of the solve (msfl_set_outlier_rejection) ----
    def set_outlier_rejection(self, threshold=None, fraction=None, which=REJECT_LAST_OUTER, n=0):
        """Every later matcher call rejects correspondences in front of the selected solves: those whose loss-free residual norm exceeds
        `threshold`, or the ceil(n * fraction) largest of each scan.  n > 0: one msfl_rejection_record per registration goes to a host
        buffer of `n` records owned by this object (read it with rejection())."""
        cfg = outlier_rejection(threshold, fraction, which)
        self._set_sink("rejection", lambda p, cap, mem: self.lib.msfl_set_outlier_rejection(self.h, C.byref(cfg), p, cap, mem),
                       "msfl_set_outlier_rejection", capacity=n)

    def set_outlier_rejection_device(self, ptr, capacity, threshold=None, fraction=None, which=REJECT_LAST_OUTER):
        """Device-pointer sink: `ptr` (torch tensor / raw pointer) holds `capacity` records of REJECTION_DTYPE.itemsize bytes, written
        asynchronously on the handle's stream."""
        cfg = outlier_rejection(threshold, fraction, which)
        self._set_sink("rejection", lambda p, cap, mem: self.lib.msfl_set_outlier_rejection(self.h, C.byref(cfg), p, cap, mem),
                       "msfl_set_outlier_rejection(device)", ptr, capacity, MEM_DEVICE)

    def clear_outlier_rejection(self):
        self._set_sink("rejection", lambda p, cap, mem: self.lib.msfl_set_outlier_rejection(self.h, None, p, cap, mem),
                       "msfl_set_outlier_rejection")

    def rejection(self, n=None):
        """The first `n` records (default: all) the last matcher call wrote, as a copy of the numpy structured array."""
        return self._records("rejection", n)

    def degeneracy(self, n=None):
        """The first `n` records (default: all) the last matcher call wrote, as a copy of the numpy structured array."""
        return self._records("degeneracy", n)

    # ---- pose priors (msfl_set_pose_prior) ----
    def set_pose_prior(self, poses, sqrt_info):
        """priors[b] = (poses[b], sqrt_info[b]) joins the problem of registration b of every later matcher call.  The records
        live in a host buffer owned by this object (the library reads it at each call)."""
        rec = pose_priors(poses, sqrt_info)
        self._check(self.lib.msfl_set_pose_prior(self.h, _vp(rec), len(rec), MEM_HOST), "msfl_set_pose_prior")
        self._prior = rec

    def set_pose_prior_device(self, ptr, count):
        """Device-pointer variant: `ptr` (torch tensor / raw pointer) holds `count` records of POSE_PRIOR_DTYPE.itemsize bytes, read on
        the handle's stream at each matcher call."""
        self._check(self.lib.msfl_set_pose_prior(self.h, _vp(ptr), int(count), MEM_DEVICE), "msfl_set_pose_prior(device)")
        self._prior = ptr

    def clear_pose_prior(self):
        self._check(self.lib.msfl_set_pose_prior(self.h, None, 0, MEM_HOST), "msfl_set_pose_prior")
        self._prior = None

    # ---- stage C ----
    def set_map(self, corner, surf, n_corner=None, n_surf=None, mem=MEM_HOST):
        if mem == MEM_HOST:
            corner, surf = _pts(corner), _pts(surf)
            n_corner, n_surf = len(corner), len(surf)
            self._keep = (corner, surf)
        self._check(self.lib.msfl_set_map(self.h, _vp(corner), n_corner, _vp(surf), n_surf, mem), "msfl_set_map")

    def match_scan2map(self, corner, surf, pose, want_info=True, allow=()):
        corner, surf = _pts(corner), _pts(surf)
        pose = np.array(pose, dtype=np.float64)
        info = MatchInfo()
        s = self.lib.msfl_match_scan2map(self.h, _vp(corner), len(corner), _vp(surf), len(surf), _vp(pose), C.byref(info) if want_info else None,
                                         MEM_HOST)
        self._check(s, "msfl_match_scan2map", allow)
        return s, pose, info

    def match_scan2map_batch(self, corner, corner_off, surf, surf_off, poses, want_info=False):
        """Host-memory batch. Returns (poses (B,7), status (B,), info list or None)."""
        corner, surf = _pts(corner), _pts(surf)
        co = np.ascontiguousarray(corner_off, dtype=np.int32)
        so = np.ascontiguousarray(surf_off, dtype=np.int32)
        poses = np.array(poses, dtype=np.float64).reshape(-1, 7).copy()
        B = len(poses)
        status = np.zeros(B, np.int32)
        info = (MatchInfo * B)() if want_info else None
        s = self.lib.msfl_match_scan2map_batch(self.h, B, _vp(corner), _vp(co), _vp(surf), _vp(so), _vp(poses), _vp(status), info, MEM_HOST)
        self._check(s, "msfl_match_scan2map_batch")
        return poses, status, info

    def match_scan2map_batch_device(self, B, corner_ptr, corner_off, surf_ptr, surf_off, poses_ptr, status_ptr=None):
        """Device-resident batch (asynchronous on the handle's stream). Offsets are host arrays."""
        co = np.ascontiguousarray(corner_off, dtype=np.int32)
        so = np.ascontiguousarray(surf_off, dtype=np.int32)
        s = self.lib.msfl_match_scan2map_batch(self.h, B, _vp(corner_ptr), _vp(co), _vp(surf_ptr), _vp(so), _vp(poses_ptr), _vp(status_ptr), None,
                                               MEM_DEVICE)
        self._check(s, "msfl_match_scan2map_batch(device)")

    def match_scan2map_deskew_batch(self, corner, corner_off, surf, surf_off, corner_dq, corner_dp, surf_dq, surf_dp,
                                    velocity, gravity, poses, mem=MEM_HOST, status=None):
        """Deskew branch for B scans.  Host memory: numpy arrays in, (poses, status) out.  Device memory: pass
        tensors / pointers (poses updated in place, `status` a device int32 buffer or None)."""
        co = np.ascontiguousarray(corner_off, dtype=np.int32)
        so = np.ascontiguousarray(surf_off, dtype=np.int32)
        B = len(co) - 1
        d = DeskewBatch()
        if mem == MEM_HOST:
            corner, surf = _pts(corner), _pts(surf)
            keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (corner_dq, corner_dp, surf_dq, surf_dp, velocity)]
            poses = np.array(poses, dtype=np.float64).reshape(-1, 7).copy()
            status = np.zeros(B, np.int32)
        else:
            keep = [corner_dq, corner_dp, surf_dq, surf_dp, velocity]
        d.corner_dq, d.corner_dp, d.surf_dq, d.surf_dp, d.velocity = (_vp(a).value for a in keep)
        d.gravity = (C.c_double * 3)(*[float(g) for g in gravity])
        s = self.lib.msfl_match_scan2map_deskew_batch(self.h, B, _vp(corner), _vp(co), _vp(surf), _vp(so), C.byref(d), _vp(poses), _vp(status), None,
                                                      mem)
        self._check(s, "msfl_match_scan2map_deskew_batch")
        return poses, status

    def associate_scan2map(self, corner, surf, pose):
        """One data-association pass at `pose`: (n_corner+n_surf, 6) records {C, N}."""
        corner, surf = _pts(corner), _pts(surf)
        rec = np.zeros((max(len(corner) + len(surf), 1), 6))
        pose = np.ascontiguousarray(pose, dtype=np.float64)
        self._check(self.lib.msfl_associate_scan2map(self.h, _vp(corner), len(corner), _vp(surf), len(surf), _vp(pose), _vp(rec)),
                    "msfl_associate_scan2map")
        return rec[:len(corner) + len(surf)]

    def solve_records(self, corner, surf, records, pose):
        corner, surf = _pts(corner), _pts(surf)
        rec = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 6)
        pose = np.array(pose, dtype=np.float64)
        info = MatchInfo()
        self._check(self.lib.msfl_solve_records(self.h, _vp(corner), len(corner), _vp(surf), len(surf), _vp(rec), _vp(pose), C.byref(info)),
                    "msfl_solve_records")
        return pose, info

    def associate_scan2map_deskew(self, corner, surf, corner_dq, corner_dp, surf_dq, surf_dp, velocity, gravity, pose):
        """One de-skew association pass at `pose`: ((n, 6) records {C', N}, (n, 3) points p'), corner features first."""
        corner, surf = _pts(corner), _pts(surf)
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (corner_dq, corner_dp, surf_dq, surf_dp)]
        d = Deskew()
        d.corner_dq, d.corner_dp, d.surf_dq, d.surf_dp = (a.ctypes.data for a in arrs)
        d.velocity = (C.c_double * 3)(*velocity)
        d.gravity = (C.c_double * 3)(*gravity)
        n = len(corner) + len(surf)
        rec, pts = np.zeros((max(n, 1), 6)), np.zeros((max(n, 1), 3))
        pose = np.ascontiguousarray(pose, dtype=np.float64)
        self._check(self.lib.msfl_associate_scan2map_deskew(self.h, _vp(corner), len(corner), _vp(surf), len(surf), C.byref(d), _vp(pose), _vp(rec),
                                                            _vp(pts)), "msfl_associate_scan2map_deskew")
        return rec[:n], pts[:n]

    def solve_records_deskew(self, corner, surf, records, points, pose):
        """msfl_solve_records with the residual points given as f64 `points` (n, 3): the solve's de-skew branch."""
        corner, surf = _pts(corner), _pts(surf)
        rec = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 6)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        if len(pts) != len(corner) + len(surf) or len(rec) != len(pts):
            raise ValueError("records and points need one row per feature")
        if len(pts) == 0:
            pts = np.zeros((1, 3))                                # (the entry wants a non-null pointer)
        pose = np.array(pose, dtype=np.float64)
        info = MatchInfo()
        self._check(self.lib.msfl_solve_records_deskew(self.h, _vp(corner), len(corner), _vp(surf), len(surf), _vp(rec), _vp(pts), _vp(pose),
                                                       C.byref(info)), "msfl_solve_records_deskew")
        return pose, info

    def match_scan2map_deskew(self, corner, surf, corner_dq, corner_dp, surf_dq, surf_dp, velocity, gravity, pose):
        corner, surf = _pts(corner), _pts(surf)
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (corner_dq, corner_dp, surf_dq, surf_dp)]
        d = Deskew()
        d.corner_dq, d.corner_dp, d.surf_dq, d.surf_dp = (a.ctypes.data for a in arrs)
        d.velocity = (C.c_double * 3)(*velocity)
        d.gravity = (C.c_double * 3)(*gravity)
        pose = np.array(pose, dtype=np.float64)
        info = MatchInfo()
        s = self.lib.msfl_match_scan2map_deskew(self.h, _vp(corner), len(corner), _vp(surf), len(surf), C.byref(d), _vp(pose), C.byref(info))
        self._check(s, "msfl_match_scan2map_deskew")
        return s, pose, info

    # ---- stage B ----
    def match_scan2scan(self, last_ls, last_ls_ring, last_lf, last_lf_ring, sharp, flat, pose, allow=(TOO_FEW_CORRESPONDENCES,)):
        clouds = []
        keep = []
        for pts, ring in ((last_ls, last_ls_ring), (last_lf, last_lf_ring), (sharp, None), (flat, None)):
            p = _pts(pts)
            r = np.ascontiguousarray(ring if ring is not None else np.zeros(len(p)), dtype=np.uint16)
            keep.append((p, r))
            rc = RingCloud()
            rc.pts, rc.ring, rc.n = p.ctypes.data, r.ctypes.data, len(p)
            clouds.append(rc)
        pose = np.array(pose, dtype=np.float64)
        info = MatchInfo()
        s = self.lib.msfl_match_scan2scan(self.h, C.byref(clouds[0]), C.byref(clouds[1]), C.byref(clouds[2]), C.byref(clouds[3]), _vp(pose),
                                          C.byref(info), MEM_HOST)
        self._check(s, "msfl_match_scan2scan", allow)
        return s, pose, info

    def match_scan2scan_batch(self, clouds, poses, want_info=False):
        """clouds: 4 tuples (pts (n,4), ring (n,), off (B+1,)) for last_less_sharp, last_less_flat,
        curr_sharp, curr_flat (ring may be None for the curr sets)."""
        structs, keep = [], []
        for pts, ring, off in clouds:
            p = _pts(pts)
            r = np.ascontiguousarray(ring if ring is not None else np.zeros(len(p)), dtype=np.uint16)
            o = np.ascontiguousarray(off, dtype=np.int32)
            keep.append((p, r, o))
            rb = RingCloudBatch()
            rb.pts, rb.ring, rb.off = p.ctypes.data, r.ctypes.data, o.ctypes.data
            structs.append(rb)
        poses = np.array(poses, dtype=np.float64).reshape(-1, 7).copy()
        B = len(poses)
        status = np.zeros(B, np.int32)
        info = (MatchInfo * B)() if want_info else None
        s = self.lib.msfl_match_scan2scan_batch(self.h, B, C.byref(structs[0]), C.byref(structs[1]), C.byref(structs[2]), C.byref(structs[3]),
                                                _vp(poses), _vp(status), info, MEM_HOST)
        self._check(s, "msfl_match_scan2scan_batch")
        return poses, status, info

    # ---- stage A ----
    def extract_features(self, pts, ring, extrinsic=None, allow=()):
        pts = _pts(pts)
        ring = np.ascontiguousarray(ring, dtype=np.uint16)
        n = max(len(pts), 1)
        out = dict(full=np.zeros((n, 4), np.float32), ring=np.zeros(n, np.uint16), curvature=np.zeros(n, np.float32),
                   label=np.zeros(n, np.uint8), sharp=np.zeros(n, np.int32), less_sharp=np.zeros(n, np.int32),
                   flat=np.zeros(n, np.int32), less_flat=np.zeros(n, np.int32))
        f = Features()
        f.full_pts, f.full_ring, f.curvature, f.label = (out[k].ctypes.data for k in ("full", "ring", "curvature", "label"))
        f.sharp_idx, f.less_sharp_idx, f.flat_idx, f.less_flat_idx = (out[k].ctypes.data for k in ("sharp", "less_sharp", "flat", "less_flat"))
        ext = np.ascontiguousarray(extrinsic, dtype=np.float64) if extrinsic is not None else None
        s = self.lib.msfl_extract_features(self.h, _vp(pts), _vp(ring), len(pts), _vp(ext), C.byref(f), MEM_HOST)
        self._check(s, "msfl_extract_features", allow)
        nf = f.n_full
        return dict(rc=s, full=out["full"][:nf], ring=out["ring"][:nf], curvature=out["curvature"][:nf],
                    label=out["label"][:nf], sharp=out["sharp"][:f.n_sharp].copy(),
                    less_sharp=out["less_sharp"][:f.n_less_sharp].copy(), flat=out["flat"][:f.n_flat].copy(),
                    less_flat=out["less_flat"][:f.n_less_flat].copy())

    def extract_features_batch(self, pts, ring, off):
        """Host-memory batch.  Returns a list of per-scan dicts like extract_features()."""
        pts = _pts(pts)
        ring = np.ascontiguousarray(ring, dtype=np.uint16)
        off = np.ascontiguousarray(off, dtype=np.int32)
        B = len(off) - 1
        n = max(len(pts), 1)
        out = dict(full=np.zeros((n, 4), np.float32), ring=np.zeros(n, np.uint16), curvature=np.zeros(n, np.float32),
                   label=np.zeros(n, np.uint8), sharp=np.zeros(n, np.int32), less_sharp=np.zeros(n, np.int32),
                   flat=np.zeros(n, np.int32), less_flat=np.zeros(n, np.int32))
        cnt = {k: np.zeros(max(B, 1), np.int32) for k in ("n_full", "n_sharp", "n_less_sharp", "n_flat", "n_less_flat")}
        f = FeaturesBatch()
        f.full_pts, f.full_ring, f.curvature, f.label = (out[k].ctypes.data for k in ("full", "ring", "curvature", "label"))
        f.sharp_idx, f.less_sharp_idx, f.flat_idx, f.less_flat_idx = (out[k].ctypes.data for k in ("sharp", "less_sharp", "flat", "less_flat"))
        f.n_full, f.n_sharp, f.n_less_sharp, f.n_flat, f.n_less_flat = (cnt[k].ctypes.data for k in ("n_full", "n_sharp", "n_less_sharp", "n_flat", "n_less_flat"))
        status = np.zeros(max(B, 1), np.int32)
        s = self.lib.msfl_extract_features_batch(self.h, B, _vp(pts), _vp(ring), _vp(off), C.byref(f), _vp(status), MEM_HOST)
        self._check(s, "msfl_extract_features_batch")
        res = []
        for b in range(B):
            o = int(off[b])
            nf = int(cnt["n_full"][b])
            res.append(dict(rc=int(status[b]), full=out["full"][o:o + nf], ring=out["ring"][o:o + nf],
                            curvature=out["curvature"][o:o + nf], label=out["label"][o:o + nf],
                            sharp=out["sharp"][o:o + cnt["n_sharp"][b]].copy(),
                            less_sharp=out["less_sharp"][o:o + cnt["n_less_sharp"][b]].copy(),
                            flat=out["flat"][o:o + cnt["n_flat"][b]].copy(),
                            less_flat=out["less_flat"][o:o + cnt["n_less_flat"][b]].copy()))
        return res

    def voxel_downsample(self, pts, leaf):
        pts = _pts(pts)
        out = np.zeros((max(len(pts), 1), 4), np.float32)
        n_out = C.c_int(0)
        self._check(self.lib.msfl_voxel_downsample(self.h, _vp(pts), len(pts), leaf, _vp(out), C.byref(n_out), MEM_HOST), "msfl_voxel_downsample")
        return out[:n_out.value].copy()

    def voxel_downsample_batch(self, pts, off, leaf, idx=None, count=None):
        """Host-memory batch: clouds pts[off[b] (+ idx)] -> (filtered points back to back, out_off (B+1))."""
        pts = _pts(pts)
        off = np.ascontiguousarray(off, np.int32)
        B = len(off) - 1
        out = np.zeros((max(int(off[-1] - off[0]), 1), 4), np.float32)
        out_off = np.zeros(B + 1, np.int32)
        idx_a = None if idx is None else np.ascontiguousarray(idx, np.int32)
        cnt_a = None if count is None else np.ascontiguousarray(count, np.int32)
        self._check(self.lib.msfl_voxel_downsample_batch(self.h, B, _vp(pts), _vp(idx_a) if idx_a is not None else None, _vp(off),
                                                         _vp(cnt_a) if cnt_a is not None else None, leaf, _vp(out), _vp(out_off), MEM_HOST),
                    "msfl_voxel_downsample_batch")
        return out[:out_off[-1]].copy(), out_off

    def match_pairs_batch(self, map_corner, map_corner_off, map_surf, map_surf_off, corner, corner_off, surf, surf_off, poses, want_info=False):
        """P (map, scan) pairs with distinct maps in one call (host memory) -> (poses (P,7), status (P,), info list or None)."""
        mc, ms, c, s_ = _pts(map_corner), _pts(map_surf), _pts(corner), _pts(surf)
        offs = [np.ascontiguousarray(o, np.int32) for o in (map_corner_off, map_surf_off, corner_off, surf_off)]
        P = len(offs[0]) - 1
        poses = np.ascontiguousarray(np.array(poses, np.float64).reshape(P, 7))
        status = np.zeros(P, np.int32)
        info = (MatchInfo * P)() if want_info else None
        self._check(self.lib.msfl_match_pairs_batch(self.h, P, _vp(mc), _vp(offs[0]), _vp(ms), _vp(offs[1]), _vp(c), _vp(offs[2]), _vp(s_),
                                                    _vp(offs[3]), _vp(poses), _vp(status), info, MEM_HOST), "msfl_match_pairs_batch")
        return poses, status, info

    def match_pairs_batch_device(self, P, d_map_corner, map_corner_off, d_map_surf, map_surf_off, d_corner, corner_off, d_surf, surf_off,
                                 d_poses, d_status):
        """The same with device-resident clouds / poses / status (torch tensors or raw pointers) and host offset arrays; asynchronous."""
        offs = [np.ascontiguousarray(o, np.int32) for o in (map_corner_off, map_surf_off, corner_off, surf_off)]
        self._keep_offs = offs
        self._check(self.lib.msfl_match_pairs_batch(self.h, P, _vp(d_map_corner), _vp(offs[0]), _vp(d_map_surf), _vp(offs[1]), _vp(d_corner),
                                                    _vp(offs[2]), _vp(d_surf), _vp(offs[3]), _vp(d_poses), _vp(d_status), None, MEM_DEVICE),
                    "msfl_match_pairs_batch(device)")

    # ---- resident pair maps (msfl_set_pair_maps, msfl_match_pairs_resident; msfl_score_pairs is with the pose scoring below) ----
    def set_pair_maps(self, map_corner, map_corner_off, map_surf, map_surf_off):
        """The index half of match_pairs_batch (host memory): the P maps indexed, one grid per pair, and kept resident for
        score_pairs and match_pairs_resident until set_map, the next set_pair_maps or the next match_pairs_batch."""
        mc, ms = _pts(map_corner), _pts(map_surf)
        offs = [np.ascontiguousarray(o, np.int32) for o in (map_corner_off, map_surf_off)]
        self._check(self.lib.msfl_set_pair_maps(self.h, len(offs[0]) - 1, _vp(mc), _vp(offs[0]), _vp(ms), _vp(offs[1]), MEM_HOST),
                    "msfl_set_pair_maps")

    def set_pair_maps_device(self, P, d_map_corner, map_corner_off, d_map_surf, map_surf_off):
        """The same with device-resident map clouds (torch tensors or raw pointers) and host offset arrays; asynchronous."""
        offs = [np.ascontiguousarray(o, np.int32) for o in (map_corner_off, map_surf_off)]
        self._check(self.lib.msfl_set_pair_maps(self.h, int(P), _vp(d_map_corner), _vp(offs[0]), _vp(d_map_surf), _vp(offs[1]), MEM_DEVICE),
                    "msfl_set_pair_maps(device)")

    def match_pairs_resident(self, corner, corner_off, surf, surf_off, poses, want_info=False):
        """The registration half of match_pairs_batch against the resident pair index (host memory) -> (poses (P,7), status (P,),
        info list or None).  The index is not consumed."""
        c, s_ = _pts(corner), _pts(surf)
        offs = [np.ascontiguousarray(o, np.int32) for o in (corner_off, surf_off)]
        P = len(offs[0]) - 1
        poses = np.ascontiguousarray(np.array(poses, np.float64).reshape(P, 7))
        status = np.zeros(P, np.int32)
        info = (MatchInfo * P)() if want_info else None
        self._check(self.lib.msfl_match_pairs_resident(self.h, P, _vp(c), _vp(offs[0]), _vp(s_), _vp(offs[1]), _vp(poses), _vp(status), info,
                                                       MEM_HOST), "msfl_match_pairs_resident")
        return poses, status, info

    def match_pairs_resident_device(self, P, d_corner, corner_off, d_surf, surf_off, d_poses, d_status):
        """The same with device-resident clouds / poses / status and host offset arrays; asynchronous."""
        offs = [np.ascontiguousarray(o, np.int32) for o in (corner_off, surf_off)]
        self._check(self.lib.msfl_match_pairs_resident(self.h, int(P), _vp(d_corner), _vp(offs[0]), _vp(d_surf), _vp(offs[1]), _vp(d_poses),
                                                       _vp(d_status), None, MEM_DEVICE), "msfl_match_pairs_resident(device)")

    # ---- pose scoring (msfl_score_poses, msfl_score_pairs) ----
    def score_poses_device(self, corner, n_corner, surf, n_surf, poses, n_poses, max_dist, scores, d2_out=None, nn_out=None):
        """Device-pointer form (torch tensors / raw pointers), asynchronous on the handle's stream: `scores` holds n_poses records of
        POSE_SCORE_DTYPE.itemsize bytes, d2_out / nn_out (optional) n_poses x (n_corner + n_surf) float32 / int32."""
        self._check(self.lib.msfl_score_poses(self.h, _vp(corner), int(n_corner), _vp(surf), int(n_surf), _vp(poses), int(n_poses), max_dist,
                                              _vp(scores), _vp(d2_out), _vp(nn_out), MEM_DEVICE), "msfl_score_poses(device)")

    def score_poses_batch_device(self, n_scans, corner, corner_off, surf, surf_off, poses, pose_off, max_dist, scores):
        """Device-pointer batch form, asynchronous; the three offset arrays are host arrays."""
        offs = [np.ascontiguousarray(o, np.int32) for o in (corner_off, surf_off, pose_off)]
        self._check(self.lib.msfl_score_poses_batch(self.h, int(n_scans), _vp(corner), _vp(offs[0]), _vp(surf), _vp(offs[1]), _vp(poses),
                                                    _vp(offs[2]), max_dist, _vp(scores), MEM_DEVICE), "msfl_score_poses_batch(device)")

    def _device_scores(self, like, n):
        import torch
        return torch.empty(max(int(n), 1) * POSE_SCORE_DTYPE.itemsize, dtype=torch.uint8, device=like.device)

    @staticmethod
    def _device_inputs(corner, surf, poses):
        import torch
        if not (_on_device(corner) and _on_device(surf) and _on_device(poses)):
            raise TypeError("score_poses: clouds and poses must all be device tensors, or none of them")
        if corner.dtype != torch.float32 or surf.dtype != torch.float32 or poses.dtype != torch.float64:
            raise TypeError("score_poses: device clouds are float32, device poses float64")
        return corner.contiguous(), surf.contiguous(), poses.contiguous()

    @staticmethod
    def _scores_to_host(buf, n):
        return buf.cpu().numpy().view(POSE_SCORE_DTYPE)[:int(n)].copy()

    def score_poses(self, corner, surf, poses, max_dist, want_nn=False):
        """Fitness of one scan at each of `poses` (P, 7) against the resident map: P records of POSE_SCORE_DTYPE (see fitness() and
        rmse()).  want_nn: also (d2, nn), each (P, n_corner + n_surf), corner features first: squared distance and original map index
        of every feature's nearest map point of its kind (+inf / -1 without one within max_dist).  numpy arrays go through host
        memory; torch device tensors (float32 (n, 4) clouds, float64 poses) through the device form on the handle's stream."""
        if _on_device(corner) or _on_device(surf) or _on_device(poses):
            import torch
            corner, surf, poses = self._device_inputs(corner, surf, poses)
            nc, ns, P = corner.numel() // 4, surf.numel() // 4, poses.numel() // 7
            buf = self._device_scores(poses, P)
            d2 = torch.empty((P, nc + ns), dtype=torch.float32, device=poses.device) if want_nn else None
            nn = torch.empty((P, nc + ns), dtype=torch.int32, device=poses.device) if want_nn else None
            self.score_poses_device(corner, nc, surf, ns, poses, P, max_dist, buf, d2, nn)
            self.synchronize()
            rec = self._scores_to_host(buf, P)
            return (rec, d2.cpu().numpy(), nn.cpu().numpy()) if want_nn else rec
        corner, surf = _pts(corner), _pts(surf)
        poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 7))
        P, F = len(poses), len(corner) + len(surf)
        rec = np.zeros(P, POSE_SCORE_DTYPE)
        d2 = np.zeros((P, F), np.float32) if want_nn else None
        nn = np.zeros((P, F), np.int32) if want_nn else None
        self._check(self.lib.msfl_score_poses(self.h, _vp(corner), len(corner), _vp(surf), len(surf), _vp(poses), P, max_dist, _vp(rec), _vp(d2),
                                              _vp(nn), MEM_HOST), "msfl_score_poses")
        return (rec, d2, nn) if want_nn else rec

    def score_poses_batch(self, corner, corner_off, surf, surf_off, poses, pose_off, max_dist):
        """Scan b (features [corner_off[b], corner_off[b+1]) / surf likewise) at the poses [pose_off[b], pose_off[b+1]): one record of
        POSE_SCORE_DTYPE per pose.  Offsets are host arrays; clouds and poses numpy arrays or, all three, torch device tensors."""
        offs = [np.ascontiguousarray(o, np.int32) for o in (corner_off, surf_off, pose_off)]
        B = len(offs[0]) - 1
        if _on_device(corner) or _on_device(surf) or _on_device(poses):
            corner, surf, poses = self._device_inputs(corner, surf, poses)
            P = poses.numel() // 7
            buf = self._device_scores(poses, P)
            self.score_poses_batch_device(B, corner, offs[0], surf, offs[1], poses, offs[2], max_dist, buf)
            self.synchronize()
            rec = np.zeros(P, POSE_SCORE_DTYPE)                     # poses outside [pose_off[0], pose_off[B]) keep zero records
            p0, p1 = (int(offs[2][0]), int(offs[2][-1])) if B > 0 else (0, 0)
            rec[p0:p1] = self._scores_to_host(buf, P)[p0:p1]
            return rec
        corner, surf = _pts(corner), _pts(surf)
        poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 7))
        rec = np.zeros(len(poses), POSE_SCORE_DTYPE)
        self._check(self.lib.msfl_score_poses_batch(self.h, B, _vp(corner), _vp(offs[0]), _vp(surf), _vp(offs[1]), _vp(poses), _vp(offs[2]), max_dist,
                                                    _vp(rec), MEM_HOST), "msfl_score_poses_batch")
        return rec

    def score_pairs_device(self, n_pairs, corner, corner_off, surf, surf_off, poses, pose_off, max_dist, scores, d2_out=None, nn_out=None):
        """Device-pointer form of score_pairs, asynchronous; the three offset arrays are host arrays.  d2_out / nn_out (optional):
        sum over the pairs of poses x features float32 / int32, ragged rows in pose order."""
        offs = [np.ascontiguousarray(o, np.int32) for o in (corner_off, surf_off, pose_off)]
        self._check(self.lib.msfl_score_pairs(self.h, int(n_pairs), _vp(corner), _vp(offs[0]), _vp(surf), _vp(offs[1]), _vp(poses), _vp(offs[2]),
                                              max_dist, _vp(scores), _vp(d2_out), _vp(nn_out), MEM_DEVICE), "msfl_score_pairs(device)")

    def score_pairs(self, corner, corner_off, surf, surf_off, poses, pose_off, max_dist, want_nn=False):
        """score_poses_batch against the resident PAIR index (set_pair_maps, or what match_pairs_batch left): scan p at the poses
        [pose_off[p], pose_off[p+1]) against pair map p only; one record of POSE_SCORE_DTYPE per pose.  want_nn: also (d2, nn), flat
        and ragged: the row of a pose of scan p has that scan's n_corner + n_surf values, rows in pose order; nn is the position in
        pair p's own map cloud of the feature's kind.  Offsets are host arrays; clouds and poses numpy arrays or, all three, torch
        device tensors."""
        offs = [np.ascontiguousarray(o, np.int32) for o in (corner_off, surf_off, pose_off)]
        B = len(offs[0]) - 1
        n_out = int(sum(int(offs[2][b + 1] - offs[2][b]) * int(offs[0][b + 1] - offs[0][b] + offs[1][b + 1] - offs[1][b]) for b in range(B)))
        if _on_device(corner) or _on_device(surf) or _on_device(poses):
            import torch
            corner, surf, poses = self._device_inputs(corner, surf, poses)
            P = poses.numel() // 7
            buf = self._device_scores(poses, P)
            d2 = torch.empty(max(n_out, 1), dtype=torch.float32, device=poses.device) if want_nn else None
            nn = torch.empty(max(n_out, 1), dtype=torch.int32, device=poses.device) if want_nn else None
            self.score_pairs_device(B, corner, offs[0], surf, offs[1], poses, offs[2], max_dist, buf, d2, nn)
            self.synchronize()
            rec = np.zeros(P, POSE_SCORE_DTYPE)                     # poses outside [pose_off[0], pose_off[B]) keep zero records
            p0, p1 = (int(offs[2][0]), int(offs[2][-1])) if B > 0 else (0, 0)
            rec[p0:p1] = self._scores_to_host(buf, P)[p0:p1]
            return (rec, d2.cpu().numpy()[:n_out], nn.cpu().numpy()[:n_out]) if want_nn else rec
        corner, surf = _pts(corner), _pts(surf)
        poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 7))
        rec = np.zeros(len(poses), POSE_SCORE_DTYPE)
        d2 = np.zeros(n_out, np.float32) if want_nn else None
        nn = np.zeros(n_out, np.int32) if want_nn else None
        self._check(self.lib.msfl_score_pairs(self.h, B, _vp(corner), _vp(offs[0]), _vp(surf), _vp(offs[1]), _vp(poses), _vp(offs[2]), max_dist,
                                              _vp(rec), _vp(d2), _vp(nn), MEM_HOST), "msfl_score_pairs")
        return (rec, d2, nn) if want_nn else rec

    # ---- pose search (msfl_search_poses, msfl_relocalize) ----
    def search_poses_device(self, corner, n_corner, surf, n_surf, guess, config, candidates, capacity, n_out, hits_out=None):
        """Device-pointer form, asynchronous on the handle's stream: `candidates` holds capacity records of POSE_CANDIDATE_DTYPE.itemsize
        bytes, n_out one int32, hits_out (optional) 2 x H int32; guess (7 doubles) and config are host data."""
        guess = np.ascontiguousarray(np.asarray(guess, np.float64).reshape(7))
        self._check(self.lib.msfl_search_poses(self.h, _vp(corner), int(n_corner), _vp(surf), int(n_surf), _vp(guess), C.byref(config),
                                               _vp(candidates), int(capacity), _vp(n_out), _vp(hits_out), MEM_DEVICE), "msfl_search_poses(device)")

    def search_poses(self, corner, surf, guess, config=None, capacity=16, want_hits=False):
        """The best `capacity` peaks of the hit-count lattice round `guess` (include/msfl_c_api.h, docs/kernels/search.md): records of
        POSE_CANDIDATE_DTYPE, best first.  want_hits: also hits (2, H) int32 over the whole lattice.  numpy clouds go through host
        memory, torch device tensors (float32 (n, 4)) through the device form."""
        config = SearchConfig() if config is None else config
        guess = np.ascontiguousarray(np.asarray(guess, np.float64).reshape(7))
        if _on_device(corner) or _on_device(surf):
            import torch
            if not (_on_device(corner) and _on_device(surf)) or corner.dtype != torch.float32 or surf.dtype != torch.float32:
                raise TypeError("search_poses: both clouds must be float32 device tensors, or neither")
            corner, surf = corner.contiguous(), surf.contiguous()
            nc, ns = corner.numel() // 4, surf.numel() // 4
            _, geom = search_geometry(guess, config, nc, ns, allow=(BAD_ARG, CAPACITY))     # (the call itself refuses those)
            cand = torch.zeros(max(int(capacity), 1) * POSE_CANDIDATE_DTYPE.itemsize, dtype=torch.uint8, device=corner.device)
            n_out = torch.zeros(1, dtype=torch.int32, device=corner.device)
            hits = torch.zeros((2, max(int(geom.n_hypotheses), 1)), dtype=torch.int32, device=corner.device) if want_hits else None
            self.search_poses_device(corner, nc, surf, ns, guess, config, cand, capacity, n_out, hits)
            self.synchronize()
            rec = cand.cpu().numpy().view(POSE_CANDIDATE_DTYPE)[:int(n_out.item())].copy()
            return (rec, hits.cpu().numpy()[:, :int(geom.n_hypotheses)]) if want_hits else rec
        corner, surf = _pts(corner), _pts(surf)
        _, geom = search_geometry(guess, config, len(corner), len(surf), allow=(BAD_ARG, CAPACITY))
        cand = np.zeros(max(int(capacity), 1), POSE_CANDIDATE_DTYPE)
        n_out = np.zeros(1, np.int32)
        hits = np.zeros((2, max(int(geom.n_hypotheses), 1)), np.int32) if want_hits else None
        self._check(self.lib.msfl_search_poses(self.h, _vp(corner), len(corner), _vp(surf), len(surf), _vp(guess), C.byref(config), _vp(cand),
                                               int(capacity), _vp(n_out), _vp(hits), MEM_HOST), "msfl_search_poses")
        rec = cand[:int(n_out[0])].copy()
        return (rec, hits[:, :int(geom.n_hypotheses)]) if want_hits else rec

    def search_pairs_device(self, n_pairs, corner, corner_off, surf, surf_off, guesses, config, candidates, capacity, n_out, hits_out=None):
        """Device-pointer form of search_pairs, asynchronous on the handle's stream: `candidates` holds n_pairs x capacity records of
        POSE_CANDIDATE_DTYPE.itemsize bytes, n_out n_pairs int32, hits_out (optional) n_pairs x 2 x H int32; the offset arrays, the
        guesses (n_pairs x 7 doubles) and config are host data."""
        offs = [np.ascontiguousarray(o, np.int32) for o in (corner_off, surf_off)]
        guesses = np.ascontiguousarray(np.asarray(guesses, np.float64).reshape(-1, 7))
        self._check(self.lib.msfl_search_pairs(self.h, int(n_pairs), _vp(corner), _vp(offs[0]), _vp(surf), _vp(offs[1]), _vp(guesses), C.byref(config),
                                               _vp(candidates), int(capacity), _vp(n_out), _vp(hits_out), MEM_DEVICE), "msfl_search_pairs(device)")

    def search_pairs(self, corner, corner_off, surf, surf_off, guesses, config=None, capacity=16, want_hits=False):
        """search_poses against the resident PAIR index (set_pair_maps, or what match_pairs_batch left): scan p round guesses[p] against
        pair map p only, all pairs in one call.  Returns a list of P arrays of POSE_CANDIDATE_DTYPE, best first; want_hits: also hits
        (P, 2, H) int32.  Offsets and guesses are host arrays; numpy clouds go through host memory, torch device tensors (float32
        (n, 4)) through the device form."""
        config = SearchConfig() if config is None else config
        offs = [np.ascontiguousarray(o, np.int32) for o in (corner_off, surf_off)]
        P = len(offs[0]) - 1
        guesses = np.ascontiguousarray(np.asarray(guesses, np.float64).reshape(-1, 7))
        if len(guesses) != P or len(offs[1]) != P + 1:
            raise ValueError("search_pairs: %d corner offsets, %d surf offsets, %d guesses" % (len(offs[0]), len(offs[1]), len(guesses)))
        K = max(int(capacity), 1)
        # (H depends on the config only; the call itself refuses what the geometry rule refuses)
        _, geom = search_geometry(guesses[0] if P else np.array([0, 0, 0, 0, 0, 0, 1.0]), config, 0, 0, allow=(BAD_ARG, CAPACITY))
        H = max(int(geom.n_hypotheses), 0) if want_hits else 0
        if H * max(P, 1) > (1 << 31):
            raise ValueError("search_pairs: want_hits asks for %d x 2 x %d counts" % (P, H))
        if _on_device(corner) or _on_device(surf):
            import torch
            if not (_on_device(corner) and _on_device(surf)) or corner.dtype != torch.float32 or surf.dtype != torch.float32:
                raise TypeError("search_pairs: both clouds must be float32 device tensors, or neither")
            corner, surf = corner.contiguous(), surf.contiguous()
            cand = torch.zeros(max(P, 1) * K * POSE_CANDIDATE_DTYPE.itemsize, dtype=torch.uint8, device=corner.device)
            n_out = torch.zeros(max(P, 1), dtype=torch.int32, device=corner.device)
            hits = torch.zeros((max(P, 1), 2, max(H, 1)), dtype=torch.int32, device=corner.device) if want_hits else None
            self.search_pairs_device(P, corner, offs[0], surf, offs[1], guesses, config, cand, capacity, n_out, hits)
            self.synchronize()
            cand = cand.cpu().numpy().view(POSE_CANDIDATE_DTYPE).reshape(max(P, 1), K)
            n_out = n_out.cpu().numpy()
            hits = hits.cpu().numpy() if want_hits else None
        else:
            corner, surf = _pts(corner), _pts(surf)
            cand = np.zeros((max(P, 1), K), POSE_CANDIDATE_DTYPE)
            n_out = np.zeros(max(P, 1), np.int32)
            hits = np.zeros((max(P, 1), 2, max(H, 1)), np.int32) if want_hits else None
            self._check(self.lib.msfl_search_pairs(self.h, P, _vp(corner), _vp(offs[0]), _vp(surf), _vp(offs[1]), _vp(guesses), C.byref(config),
                                                   _vp(cand), int(capacity), _vp(n_out), _vp(hits), MEM_HOST), "msfl_search_pairs")
        recs = [cand[p, :int(n_out[p])].copy() for p in range(P)]
        return (recs, hits[:P, :, :H]) if want_hits else recs

    def relocalize(self, corner, surf, guess, config=None, n_candidates=16, max_dist=1.0, n_refine=5, min_fitness=0.5):
        """msfl_relocalize: search, exact score, registration of the best n_refine, exact score again.  Records of RELOC_RESULT_DTYPE,
        best first (refined inliers descending, fixed-point sum ascending).  Clouds: numpy arrays, or both torch device tensors."""
        config = SearchConfig() if config is None else config
        guess = np.ascontiguousarray(np.asarray(guess, np.float64).reshape(7))
        mem = MEM_HOST
        if _on_device(corner) or _on_device(surf):
            import torch
            if not (_on_device(corner) and _on_device(surf)) or corner.dtype != torch.float32 or surf.dtype != torch.float32:
                raise TypeError("relocalize: both clouds must be float32 device tensors, or neither")
            corner, surf = corner.contiguous(), surf.contiguous()
            nc, ns, mem = corner.numel() // 4, surf.numel() // 4, MEM_DEVICE
        else:
            corner, surf = _pts(corner), _pts(surf)
            nc, ns = len(corner), len(surf)
        out = np.zeros(max(int(n_refine), 1), RELOC_RESULT_DTYPE)
        n_out = np.zeros(1, np.int32)
        self._check(self.lib.msfl_relocalize(self.h, _vp(corner), nc, _vp(surf), ns, _vp(guess), C.byref(config), int(n_candidates), float(max_dist),
                                             int(n_refine), float(min_fitness), _vp(out), len(out), _vp(n_out), mem), "msfl_relocalize")
        return out[:int(n_out[0])].copy()

    # ---- scan segmentation (msfl_segment_scans) ----
    def segment_scans_device(self, pts, ring, off, config, cls_out, segment_out=None, masked_out=None, info=None):
        """Device-pointer form: pts, ring and the three outputs are device memory (tensors or addresses), `off` (n_scans + 1) and
        `info` (None, or n_scans records of SEGMENT_INFO_DTYPE) host arrays.  Without `info` the call only enqueues."""
        off = np.ascontiguousarray(off, dtype=np.int32)
        cfg = C.byref(config) if config is not None else None
        self._check(self.lib.msfl_segment_scans(self.h, len(off) - 1, _vp(pts), _vp(ring), _vp(off), cfg, _vp(cls_out), _vp(segment_out),
                                                _vp(masked_out), _vp(info), MEM_DEVICE), "msfl_segment_scans(device)")

    def segment_scans(self, pts, ring, off, config=None, want_segment=True, want_masked=True, want_info=True):
        """msfl_segment_scans (include/msfl_c_api.h, docs/kernels/segment.md): scan b is pts[off[b]:off[b + 1]].  Returns a dict:
        cls (uint8 per point: SEG_NONE .. SEG_OUTLIER), segment (int32 component id or -1), masked (the cloud with the dropped
        points set to NaN: hand it to extract_features* or Slam.add_scan), info (records of SEGMENT_INFO_DTYPE, one per scan);
        the want_* switches leave an output out (None).  numpy arrays go through host memory; torch device tensors (pts float32
        (n, 4), ring a 16-bit integer type) through the device form, whose outputs are tensors and which does not wait for the
        device when want_info is off."""
        off = np.ascontiguousarray(off, dtype=np.int32)
        B = len(off) - 1
        info = np.zeros(max(B, 1), SEGMENT_INFO_DTYPE) if want_info else None
        if _on_device(pts) or _on_device(ring):
            import torch
            if not (_on_device(pts) and _on_device(ring)) or pts.dtype != torch.float32 or ring.element_size() != 2:
                raise TypeError("segment_scans: pts must be a float32 and ring a 16-bit device tensor, or both numpy arrays")
            pts, ring = pts.contiguous(), ring.contiguous()
            n = pts.numel() // 4
            cls = torch.zeros(max(n, 1), dtype=torch.uint8, device=pts.device)
            seg = torch.zeros(max(n, 1), dtype=torch.int32, device=pts.device) if want_segment else None
            masked = torch.zeros((max(n, 1), 4), dtype=torch.float32, device=pts.device) if want_masked else None
            self.segment_scans_device(pts, ring, off, config, cls, seg, masked, info)
            self._seg_keep = (pts, ring)                             # the inputs of an enqueued call stay alive until the next one
            return dict(cls=cls[:n], segment=None if seg is None else seg[:n], masked=None if masked is None else masked[:n],
                        info=None if info is None else info[:B])
        pts = _pts(pts)
        ring = np.ascontiguousarray(ring, dtype=np.uint16)
        n = len(pts)
        cls = np.zeros(max(n, 1), np.uint8)
        seg = np.zeros(max(n, 1), np.int32) if want_segment else None
        masked = np.zeros((max(n, 1), 4), np.float32) if want_masked else None
        cfg = C.byref(config) if config is not None else None
        self._check(self.lib.msfl_segment_scans(self.h, B, _vp(pts), _vp(ring), _vp(off), cfg, _vp(cls), _vp(seg), _vp(masked), _vp(info),
                                                MEM_HOST), "msfl_segment_scans")
        return dict(cls=cls[:n], segment=None if seg is None else seg[:n], masked=None if masked is None else masked[:n],
                    info=None if info is None else info[:B])

    def segment_scan(self, pts, ring, config=None, **kw):
        """msfl_segment_scan: one scan; segment_scans' dict with `info` one record."""
        n = (pts.numel() // 4) if _on_device(pts) else len(_pts(pts))
        out = self.segment_scans(pts, ring, [0, n], config, **kw)
        if out["info"] is not None:
            out["info"] = out["info"][0]
        return out

    # ---- scan novelty (msfl_scan_novelty) ----
    def scan_novelty(self, scan, map_img, config=None, want_masked=True, allow=()):
        """msfl_scan_novelty through host memory (docs/kernels/novelty.md): one class per point of `scan` (sensor frame) against the
        map image `map_img` (n_row x n_col f32, what Grid.render delivers).  Returns dict(cls, masked, info): cls uint8 per point
        (NOV_NONE .. NOV_IN_FRONT), masked the cloud with the dropped points set to NaN (hand it to extract_features* or
        Slam.add_scan), info a NoveltyInfo."""
        img = np.ascontiguousarray(map_img, dtype=np.float32)
        return _novelty_host(lambda s, n, c, cls, m, info: self.lib.msfl_scan_novelty(self.h, s, n, _vp(img), c, cls, m, info, MEM_HOST),
                             scan, config, want_masked, "msfl_scan_novelty", self._check, allow)

    def scan_novelty_device(self, scan_ptr, n, map_img_ptr, config, cls_ptr, masked_ptr=None, want_info=False, allow=()):
        """msfl_scan_novelty with the scan, the image and the outputs in device memory (tensors or addresses).  Without want_info
        the call only enqueues and returns None; with it the NoveltyInfo."""
        info = NoveltyInfo() if want_info else None
        cfg = C.byref(config) if config is not None else None
        s = self._check(self.lib.msfl_scan_novelty(self.h, _vp(scan_ptr), int(n), _vp(map_img_ptr), cfg, _vp(cls_ptr), _vp(masked_ptr),
                                                   C.byref(info) if want_info else None, MEM_DEVICE), "msfl_scan_novelty(device)", allow)
        if want_info:
            info.status = s
        return info

    def transform_cloud(self, pts, pose7):
        """TransformPointCloud (laser_mapping.cc:24-31)."""
        pts = _pts(pts)
        pose7 = np.ascontiguousarray(pose7, np.float64)
        out = np.zeros_like(pts)
        self._check(self.lib.msfl_transform_cloud(self.h, _vp(pts), len(pts), _vp(pose7), _vp(out), MEM_HOST), "msfl_transform_cloud")
        return out

    @staticmethod
    def _preintegration(sum_dt, delta_q, delta_p):
        keep = (np.ascontiguousarray(sum_dt, np.float64), np.ascontiguousarray(delta_q, np.float64).reshape(-1, 4),
                np.ascontiguousarray(delta_p, np.float64).reshape(-1, 3))
        pre = Preintegration(keep[0].ctypes.data_as(C.POINTER(C.c_double)), keep[1].ctypes.data_as(C.POINTER(C.c_double)),
                             keep[2].ctypes.data_as(C.POINTER(C.c_double)), len(keep[0]))
        return pre, keep

    def delta_qp(self, sum_dt, delta_q, delta_p, pts):
        """GetDeltaQP (scan_undistortion.cc:22-42) per point -> (status, dq (n,4), dp (n,3))."""
        pts = _pts(pts)
        pre, keep = self._preintegration(sum_dt, delta_q, delta_p)
        dq, dp = np.zeros((len(pts), 4)), np.zeros((len(pts), 3))
        s = self.lib.msfl_delta_qp(self.h, C.byref(pre), _vp(pts), len(pts), _vp(dq), _vp(dp), MEM_HOST)
        return s, dq, dp

    def deskew_cloud(self, sum_dt, delta_q, delta_p, pts, rot_odom_xyzw, velocity, gravity):
        """laser_mapping.cc:197-211 -> (status, deskewed points)."""
        pts = _pts(pts).copy()
        pre, keep = self._preintegration(sum_dt, delta_q, delta_p)
        r, v, g = (np.ascontiguousarray(a, np.float64) for a in (rot_odom_xyzw, velocity, gravity))
        s = self.lib.msfl_deskew_cloud(self.h, C.byref(pre), _vp(pts), len(pts), _vp(r), _vp(v), _vp(g), MEM_HOST)
        return s, pts

    def undistort_cloud(self, sum_dt, delta_q, delta_p, pts):
        """UndistortScanInternal (scan_undistortion.cc:5-19) -> (status, points)."""
        pts = _pts(pts).copy()
        pre, keep = self._preintegration(sum_dt, delta_q, delta_p)
        s = self.lib.msfl_undistort_cloud(self.h, C.byref(pre), _vp(pts), len(pts), MEM_HOST)
        return s, pts


class Grid(_Owner):
    """Device-resident local map store (HybridGrid): msfl_grid_* over a Handle's stream."""
    _PTR, _DESTROY = "g", "msfl_grid_destroy"

    def __init__(self, handle, resolution=3.0, leaf=0.2):
        self.handle = handle
        self.resolution, self.leaf = float(resolution), float(leaf)          # what the store was created with (mapio.save_grid)
        self._check(handle.lib.msfl_grid_create(handle.h, resolution, leaf, self._own(handle.lib)), "msfl_grid_create")
        handle._dependents.add(self)                                # Handle.close() closes the grids that are still open first

    def insert_scan(self, pts, allow=()):
        pts = _pts(pts)
        return self._check(self.lib.msfl_grid_insert_scan(self.g, _vp(pts), len(pts), MEM_HOST), "msfl_grid_insert_scan", allow)

    def size(self):
        a, b = C.c_int(0), C.c_int(0)
        self._check(self.lib.msfl_grid_size(self.g, C.byref(a), C.byref(b)), "msfl_grid_size")
        return a.value, b.value

    def get_surrounded(self, scan, pose):
        scan = _pts(scan)
        cap = max(self.size()[0], 1)
        out = np.zeros((cap, 4), np.float32)
        n_out = C.c_int(0)
        pose = np.ascontiguousarray(pose, dtype=np.float64)
        self._check(self.lib.msfl_grid_get_surrounded(self.g, _vp(scan), len(scan), _vp(pose), _vp(out), cap, C.byref(n_out), MEM_HOST),
                    "msfl_grid_get_surrounded")
        return out[:n_out.value].copy()

    def get_surrounded_device(self, scan_ptr, n, pose, out_ptr, capacity):
        """Device-resident variant: returns the number of points written at out_ptr."""
        n_out = C.c_int(0)
        pose = np.ascontiguousarray(pose, dtype=np.float64)
        self._check(self.lib.msfl_grid_get_surrounded(self.g, _vp(scan_ptr), n, _vp(pose), _vp(out_ptr), capacity, C.byref(n_out), MEM_DEVICE),
                    "msfl_grid_get_surrounded(device)")
        return n_out.value

    def dump(self):
        cap = max(self.size()[0], 1)
        out = np.zeros((cap, 4), np.float32)
        n_out = C.c_int(0)
        self._check(self.lib.msfl_grid_dump(self.g, _vp(out), cap, C.byref(n_out), MEM_HOST), "msfl_grid_dump")
        return out[:n_out.value].copy()

    def dump_cells(self):
        """(n_cells, 4) int32 {ix, iy, iz, count}, in the order of dump()."""
        cap = max(self.size()[1], 1)
        out = np.zeros((cap, 4), np.int32)
        n_out = C.c_int(0)
        self._check(self.lib.msfl_grid_dump_cells(self.g, _vp(out), cap, C.byref(n_out)), "msfl_grid_dump_cells")
        return out[:n_out.value].copy()

    def stats(self):
        """dict of msfl_grid_stats: n_points, n_cells, pool_top, pool_capacity_points, cell_capacity, device_bytes."""
        out = (C.c_longlong * 6)()
        self._check(self.lib.msfl_grid_stats(self.g, out), "msfl_grid_stats")
        return dict(zip(GRID_STATS, (int(v) for v in out)))

    def crop(self, center, half_cells, keep_evicted=False, capacity=None, allow=()):
        """Forget every cell outside +-half_cells cells around the cell of `center` (msfl_grid_crop).  Returns the GridCropInfo, or
        (info, evicted (m, 4) array) with keep_evicted; capacity: room for the evicted points (default: every live point).  A crop
        refused for want of room raises unless CAPACITY is in `allow` (then info.applied == 0 and the array is empty)."""
        center = (C.c_double * 3)(*[float(v) for v in center])
        half = (C.c_int * 3)(*[int(v) for v in half_cells])
        info = GridCropInfo()
        ev, cap = None, 0
        if keep_evicted:
            cap = self.size()[0] if capacity is None else int(capacity)
            ev = np.zeros((max(cap, 1), 4), np.float32)
        info.status = self._check(self.lib.msfl_grid_crop(self.g, center, half, _vp(ev), cap, MEM_HOST, C.byref(info)), "msfl_grid_crop", allow)
        if not keep_evicted:
            return info
        return info, ev[:info.n_points_evicted if info.applied else 0].copy()

    def crop_device(self, center, half_cells, evicted_ptr, capacity, allow=()):
        """msfl_grid_crop with a device buffer for the evicted points; returns the GridCropInfo."""
        center = (C.c_double * 3)(*[float(v) for v in center])
        half = (C.c_int * 3)(*[int(v) for v in half_cells])
        info = GridCropInfo()
        info.status = self._check(self.lib.msfl_grid_crop(self.g, center, half, _vp(evicted_ptr), int(capacity), MEM_DEVICE, C.byref(info)),
                                  "msfl_grid_crop(device)", allow)
        return info

    def crop_tiles(self, center, half_cells, capacity=None, cell_capacity=None, allow=()):
        """msfl_grid_crop_tiles: (GridCropInfo, evicted cells (m, 4) int32 {ix, iy, iz, count}, evicted points), the pair load_cells
        takes.  capacity / cell_capacity: room for the points / cells (default: every live one).  A refused crop raises unless
        CAPACITY is in `allow` (then info.applied == 0 and both arrays are empty)."""
        center = (C.c_double * 3)(*[float(v) for v in center])
        half = (C.c_int * 3)(*[int(v) for v in half_cells])
        info = GridCropInfo()
        n_pts, n_cells = self.size()
        cap = n_pts if capacity is None else int(capacity)
        ccap = n_cells if cell_capacity is None else int(cell_capacity)
        ev, cells = np.zeros((max(cap, 1), 4), np.float32), np.zeros((max(ccap, 1), 4), np.int32)
        info.status = self._check(self.lib.msfl_grid_crop_tiles(self.g, center, half, _vp(ev), cap, _vp(cells), ccap, MEM_HOST, C.byref(info)),
                                  "msfl_grid_crop_tiles", allow)
        ok = info.applied and info.status == OK
        return info, cells[:info.n_cells_evicted if ok else 0].copy(), ev[:info.n_points_evicted if ok else 0].copy()

    def _load(self, cells, pts_ptr, n_points, mem, allow, want_conflicts, what):
        cells = np.ascontiguousarray(np.asarray(cells, dtype=np.int32).reshape(-1, 4))
        info = GridLoadInfo()
        conflict = np.zeros(max(len(cells), 1), np.int32) if want_conflicts else None
        info.status = self._check(self.lib.msfl_grid_load_cells(self.g, _vp(cells), len(cells), pts_ptr, int(n_points), mem, _vp(conflict),
                                                                C.byref(info)), what, allow)
        return (info, conflict[:len(cells)]) if want_conflicts else info

    def load_cells(self, cells, pts, allow=(), want_conflicts=False):
        """msfl_grid_load_cells: `cells` (m, 4) {ix, iy, iz, count} and their points (n, 4), as dump_cells() / dump() or crop_tiles()
        deliver them, become live cells verbatim.  Returns the GridLoadInfo, or (info, per-cell 0/1 "already live" flags) with
        want_conflicts.  A refused load raises unless its status (BAD_ARG / CAPACITY) is in `allow`."""
        pts = _pts(pts)
        return self._load(cells, _vp(pts), len(pts), MEM_HOST, allow, want_conflicts, "msfl_grid_load_cells")

    def load_cells_device(self, cells, pts_ptr, n_points, allow=(), want_conflicts=False):
        """msfl_grid_load_cells with the points in device memory (`cells` stays a host array)."""
        return self._load(cells, _vp(pts_ptr), n_points, MEM_DEVICE, allow, want_conflicts, "msfl_grid_load_cells(device)")


    def carve(self, scan, pose, config=None, keep_removed=False, capacity=None, allow=()):
        """msfl_grid_carve: remove every stored point that `scan` (sensor frame), taken at the map pose `pose`, sees through.
        Returns (GridCarveInfo, removed): the removed points in dump() order with keep_removed, else None.  capacity: room for them
        (default: every live point).  A refused call raises unless its status is in `allow` (then info.applied == 0 and the array
        is empty)."""
        scan = _pts(scan)
        pose = np.ascontiguousarray(pose, dtype=np.float64)
        info = GridCarveInfo()
        rm, cap = None, 0
        if keep_removed:
            cap = self.size()[0] if capacity is None else int(capacity)
            rm = np.zeros((max(cap, 1), 4), np.float32)
        cfg = C.byref(config) if config is not None else None
        info.status = self._check(self.lib.msfl_grid_carve(self.g, _vp(scan), len(scan), _vp(pose), cfg, _vp(rm), cap, MEM_HOST, C.byref(info)),
                                  "msfl_grid_carve", allow)
        if not keep_removed:
            return info, None
        return info, rm[:info.n_points_removed if info.applied else 0].copy()

    def carve_device(self, scan_ptr, n, pose_ptr, config=None, removed_ptr=None, capacity=0, allow=()):
        """msfl_grid_carve with the scan, the pose (7 doubles) and the buffer for the removed points in device memory; returns the
        GridCarveInfo."""
        info = GridCarveInfo()
        cfg = C.byref(config) if config is not None else None
        info.status = self._check(self.lib.msfl_grid_carve(self.g, _vp(scan_ptr), int(n), _vp(pose_ptr), cfg, _vp(removed_ptr), int(capacity),
                                                           MEM_DEVICE, C.byref(info)), "msfl_grid_carve(device)", allow)
        return info

    def render(self, pose, config=None, image=None, accumulate=False, allow=()):
        """msfl_grid_render through host memory: the range image (n_row, n_col) f32 this store predicts for a sensor at the map pose
        `pose`, +inf where it holds nothing.  accumulate: the minimum is taken into `image` (rendered from another store before) and
        the result is a new array.  config: a CarveConfig (None: the defaults).  Returns (image, GridRenderInfo)."""
        cfg = config if config is not None else carve_config()
        pose = np.ascontiguousarray(pose, dtype=np.float64)
        if accumulate:
            img = np.array(image, dtype=np.float32, order="C", copy=True)
            if img.size != cfg.n_row * cfg.n_col:
                raise ValueError("render: `image` is not n_row x n_col")
        else:
            img = np.zeros(cfg.n_row * cfg.n_col, np.float32)
        info = GridRenderInfo()
        info.status = self._check(self.lib.msfl_grid_render(self.g, _vp(pose), C.byref(cfg), _vp(img), int(bool(accumulate)), MEM_HOST, C.byref(info)),
                                  "msfl_grid_render", allow)
        return img.reshape(cfg.n_row, cfg.n_col), info

    def render_device(self, pose_ptr, config, image_ptr, accumulate=False, want_info=False, allow=()):
        """msfl_grid_render with the pose (7 doubles) and the image in device memory.  Without want_info the call only enqueues and
        returns None; with it the GridRenderInfo."""
        info = GridRenderInfo() if want_info else None
        cfg = C.byref(config) if config is not None else None
        s = self._check(self.lib.msfl_grid_render(self.g, _vp(pose_ptr), cfg, _vp(image_ptr), int(bool(accumulate)), MEM_DEVICE,
                                                  C.byref(info) if want_info else None), "msfl_grid_render(device)", allow)
        if want_info:
            info.status = s
        return info


class _BorrowedGrid(Grid):
    """A map store owned by a Slam pipeline (never destroyed from here)."""

    def __init__(self, lib, g, err, resolution=None, leaf=None):
        self.lib, self.g, self.last_error = lib, g, err             # err: the owning pipeline's last_error
        self.resolution, self.leaf = resolution, leaf
        self.handle = self

    def close(self):
        self.g = C.c_void_p()


class KeyframesConfig(C.Structure):
    _fields_ = [("max_keyframes", C.c_int), ("max_corner_points", C.c_int), ("max_surf_points", C.c_int), ("leaf_corner", C.c_float),
                ("leaf_surf", C.c_float)]


class Keyframes(_Owner):
    """Device-resident keyframe store (msfl_keyframes_*) over a Handle's stream: the scans' corner / surf lists, laid down at any
    poses as submaps (compose) or into map stores (insert).  Keyword arguments are the fields of msfl_keyframes_config
    (max_keyframes, max_corner_points, max_surf_points, leaf_corner, leaf_surf)."""
    _PTR, _DESTROY = "k", "msfl_keyframes_destroy"

    def __init__(self, handle, **cfg):
        self.handle = handle
        ref = self._own(handle.lib)
        self.config = KeyframesConfig()
        self.lib.msfl_keyframes_default_config(C.byref(self.config))
        for k, v in cfg.items():
            if k not in dict(KeyframesConfig._fields_):
                raise TypeError("unknown msfl_keyframes_config field %r" % (k,))
            setattr(self.config, k, v)
        self._check(self.lib.msfl_keyframes_create(handle.h, C.byref(self.config), ref), "msfl_keyframes_create")
        handle._dependents.add(self)                                # Handle.close() closes what must go before the handle

    def size(self):
        return int(self.lib.msfl_keyframes_size(self.k))

    def __len__(self):
        return self.size()

    @staticmethod
    def _idx(idx):
        return None if idx is None else np.ascontiguousarray(idx, np.int32)

    def _add(self, corner, corner_idx, n_corner, surf, surf_idx, n_surf, mem, allow, what):
        index = C.c_int(-1)
        s = self._check(self.lib.msfl_keyframes_add(self.k, _vp(corner), _vp(corner_idx), int(n_corner), _vp(surf), _vp(surf_idx), int(n_surf), mem,
                                                    C.byref(index)), what, allow)
        return index.value if s == OK else s

    def add(self, corner, surf, corner_idx=None, surf_idx=None, allow=()):
        """Host memory.  With an index list the kind's list is corner[corner_idx] (the shape of Slam.clouds(): full_scan with
        less_sharp_idx / less_flat_idx).  Returns the new keyframe's index (or the refusing status when it is in `allow`)."""
        corner, surf = _pts(corner), _pts(surf)
        ci, si = self._idx(corner_idx), self._idx(surf_idx)
        return self._add(corner, ci, len(corner) if ci is None else len(ci), surf, si, len(surf) if si is None else len(si), MEM_HOST, allow,
                         "msfl_keyframes_add")

    def add_device(self, corner, n_corner, surf, n_surf, corner_idx=None, surf_idx=None, allow=()):
        """Device pointers (torch tensors / raw pointers) of 16-byte points and, optionally, of int32 index lists; n_* are the lists' sizes."""
        return self._add(corner, corner_idx, n_corner, surf, surf_idx, n_surf, MEM_DEVICE, allow, "msfl_keyframes_add(device)")

    def sizes(self, first=0, n=None):
        """-> (n_corner, n_surf) int32 arrays of keyframes [first, first + n): host bookkeeping, no device call."""
        n = self.size() - first if n is None else int(n)
        nc, ns = np.zeros(max(n, 0), np.int32), np.zeros(max(n, 0), np.int32)
        self._check(self.lib.msfl_keyframes_sizes(self.k, int(first), n, _vp(nc), _vp(ns)), "msfl_keyframes_sizes")
        return nc, ns

    def get(self, index):
        """-> (corner, surf) of one keyframe as stored."""
        nc, ns = self.sizes(index, 1)
        corner, surf = np.zeros((int(nc[0]), 4), np.float32), np.zeros((int(ns[0]), 4), np.float32)
        self._check(self.lib.msfl_keyframes_get(self.k, int(index), _vp(corner), len(corner), _vp(surf), len(surf), MEM_HOST), "msfl_keyframes_get")
        return corner, surf

    def get_device(self, index, corner, cap_corner, surf, cap_surf):
        self._check(self.lib.msfl_keyframes_get(self.k, int(index), _vp(corner), int(cap_corner), _vp(surf), int(cap_surf), MEM_DEVICE),
                    "msfl_keyframes_get(device)")

    @staticmethod
    def _members(member_off, keys, poses):
        member_off = np.ascontiguousarray(member_off, np.int32)
        keys = np.ascontiguousarray(keys, np.int32)
        poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 7))
        return member_off, keys, poses

    def member_totals(self, member_off, keys):
        """Sum of the member counts per kind over members [member_off[0], member_off[-1]): the capacities compose needs."""
        nc, ns = self.sizes()
        k = np.asarray(keys, np.int64)[int(member_off[0]):int(member_off[-1])]
        return int(nc[k].sum()), int(ns[k].sum())

    def _compose(self, member_off, keys, poses, leaf_corner, leaf_surf, out_corner, cap_corner, out_surf, cap_surf, mem, allow, what):
        B = len(member_off) - 1
        off_c, off_s = np.zeros(B + 1, np.int32), np.zeros(B + 1, np.int32)
        s = self._check(self.lib.msfl_keyframes_compose(self.k, B, _vp(member_off), _vp(keys), _vp(poses), leaf_corner, leaf_surf, _vp(out_corner),
                                                        int(cap_corner), _vp(off_c), _vp(out_surf), int(cap_surf), _vp(off_s), mem), what, allow)
        return s, off_c, off_s

    def compose(self, member_off, keys, poses, leaf_corner=0.0, leaf_surf=0.0, allow=(), out_corner=None, out_surf=None, cap_corner=None,
                cap_surf=None):
        """Host memory.  Submap b = members [member_off[b], member_off[b + 1]) of keys / poses (absolute positions), each keyframe
        transformed by its pose [t, qx qy qz qw]; leaf 0: the concatenation, else its voxel filter.  Returns
        (corner, corner_off, surf, surf_off), or the refusing status when it is in `allow`.  out_* / cap_*: the caller's arrays and
        the capacities to state (tests of the refusals); by default both come from the member counts."""
        member_off, keys, poses = self._members(member_off, keys, poses)
        if out_corner is None or out_surf is None:
            tc, ts = self.member_totals(member_off, keys)
            out_corner = np.zeros((max(tc, 1), 4), np.float32) if out_corner is None else out_corner
            out_surf = np.zeros((max(ts, 1), 4), np.float32) if out_surf is None else out_surf
        cap_corner = len(out_corner) if cap_corner is None else cap_corner
        cap_surf = len(out_surf) if cap_surf is None else cap_surf
        s, off_c, off_s = self._compose(member_off, keys, poses, leaf_corner, leaf_surf, out_corner, cap_corner, out_surf, cap_surf, MEM_HOST, allow,
                                        "msfl_keyframes_compose")
        if s != OK:
            return s
        return out_corner[:off_c[-1]].copy(), off_c, out_surf[:off_s[-1]].copy(), off_s

    def compose_device(self, member_off, keys, poses, leaf_corner, leaf_surf, out_corner, cap_corner, out_surf, cap_surf, allow=()):
        """Device outputs (torch tensors / raw pointers with room for cap_* points) -> (corner_off, surf_off) host arrays: what
        Handle.match_pairs_batch_device takes as the maps' offsets.  Asynchronous when both leaves are 0."""
        member_off, keys, poses = self._members(member_off, keys, poses)
        s, off_c, off_s = self._compose(member_off, keys, poses, leaf_corner, leaf_surf, out_corner, cap_corner, out_surf, cap_surf, MEM_DEVICE, allow,
                                        "msfl_keyframes_compose(device)")
        return (off_c, off_s) if s == OK else s

    def insert(self, keys, poses, grid_corner=None, grid_surf=None, allow=()):
        """Keyframes keys[i] at poses[i] into the given map stores (capi.Grid of the same handle; None: that kind is skipped), in
        order.  Returns (status, n_done)."""
        keys = np.ascontiguousarray(keys, np.int32)
        poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 7))
        n_done = C.c_int(0)
        s = self._check(self.lib.msfl_keyframes_insert(self.k, _vp(keys), _vp(poses), len(keys), grid_corner.g if grid_corner is not None else None,
                                                       grid_surf.g if grid_surf is not None else None, C.byref(n_done)), "msfl_keyframes_insert",
                        allow)
        return s, n_done.value


class Slam(_Owner):
    """Device-resident per-scan SLAM step (msfl_slam_*): raw scan in, poses out, everything in between stays in HBM."""
    _PTR, _DESTROY, _ERROR = "s", "msfl_slam_destroy", "msfl_slam_last_error"

    def __init__(self, device=0, max_scan_points=28800, max_rings=16, pose_odom2map=None, params=None, **cfg):
        ref = self._own(load())
        c = SlamConfig()
        self.lib.msfl_slam_default_config(C.byref(c))
        c.max_scan_points, c.max_rings = int(max_scan_points), int(max_rings)
        self.max_scan_points = int(max_scan_points)
        if pose_odom2map is not None:
            for k in range(7):
                c.pose_odom2map[k] = float(pose_odom2map[k])
        for k, v in cfg.items():
            setattr(c, k, v)
        self._grid_shape = (float(c.map_resolution), float(c.leaf_corner), float(c.leaf_surf))
        st = self.lib.msfl_slam_create(C.byref(params) if params is not None else None, C.byref(c), device, ref)
        if st != OK:
            raise MsflError(st, "msfl_slam_create", "no GPU / HIP runtime available (there is no CPU fallback)" if st == HIP_ERROR else "")
        self.n_scans = 0

    @staticmethod
    def make_imu(sum_dt, delta_q, delta_p, is_initialized=False, velocity=(0, 0, 0), gravity=(0, 0, 0), presolved_pose=None):
        """Build an msfl_slam_imu (returns (struct, keep-alive tuple)); sum_dt None = no IMU data for the scan."""
        imu = SlamImu()
        keep = None
        if sum_dt is not None:
            pre, arrays = Handle._preintegration(sum_dt, delta_q, delta_p)
            keep = (pre, arrays)
            imu.pre = C.pointer(pre)
        imu.is_initialized = 1 if is_initialized else 0
        for k in range(3):
            imu.velocity[k], imu.gravity[k] = float(velocity[k]), float(gravity[k])
        pp = presolved_pose if presolved_pose is not None else (0, 0, 0, 0, 0, 0, 1)
        for k in range(7):
            imu.presolved_pose[k] = float(pp[k])
        return imu, keep

    def add_scan(self, pts, ring, wait=True, imu=None):
        """Feed one scan (host arrays).  wait=True: returns this scan's SlamResult; False: enqueue only.
        imu: a dict of make_imu's arguments (msfl_slam_add_scan_imu), or None (LiDAR-only)."""
        pts = _pts(pts)
        ring = np.ascontiguousarray(ring, dtype=np.uint16)
        r = SlamResult() if wait else None
        if imu is None:
            st = self.lib.msfl_slam_add_scan(self.s, _vp(pts), _vp(ring), len(pts), MEM_HOST, C.byref(r) if wait else None)
        else:
            im, keep = self.make_imu(**imu)
            st = self.lib.msfl_slam_add_scan_imu(self.s, _vp(pts), _vp(ring), len(pts), MEM_HOST, C.byref(im), C.byref(r) if wait else None)
            del keep
        self._check(st, "msfl_slam_add_scan")
        self.n_scans += 1
        return r

    def add_scan_device(self, pts_ptr, ring_ptr, n, wait=True):
        r = SlamResult() if wait else None
        self._check(self.lib.msfl_slam_add_scan(self.s, _vp(pts_ptr), _vp(ring_ptr), int(n), MEM_DEVICE, C.byref(r) if wait else None),
                    "msfl_slam_add_scan(device)")
        self.n_scans += 1
        return r

    def result(self, scan_index):
        r = SlamResult()
        self._check(self.lib.msfl_slam_get_result(self.s, int(scan_index), C.byref(r)), "msfl_slam_get_result")
        return r

    def set_uncertainty(self, enabled=True, min_eigenvalue=0.0):
        self._check(self.lib.msfl_slam_set_uncertainty(self.s, 1 if enabled else 0, min_eigenvalue), "msfl_slam_set_uncertainty")

    def set_degeneracy(self, odometry=None, mapping=None):
        """Degeneracy-aware solve of every scan fed from now on: `odometry` / `mapping` is the eigenvalue threshold of that matcher,
        None leaves it off."""
        self._check(self.lib.msfl_slam_set_degeneracy(self.s, odometry is not None, mapping is not None, odometry or 0.0, mapping or 0.0),
                    "msfl_slam_set_degeneracy")

    def set_outlier_rejection(self, odometry=None, mapping=None):
        """Outlier rejection of every scan fed from now on: `odometry` / `mapping` is that matcher's OutlierRejection
        (capi.outlier_rejection(...)), None leaves it off."""
        self._check(self.lib.msfl_slam_set_outlier_rejection(self.s, None if odometry is None else C.byref(odometry),
                                                             None if mapping is None else C.byref(mapping)), "msfl_slam_set_outlier_rejection")

    def get_rejection(self, scan_index):
        """(odometry, mapping) records of REJECTION_DTYPE of one of the last four scans fed (waits for it)."""
        out = np.zeros(2, REJECTION_DTYPE)
        self._check(self.lib.msfl_slam_get_rejection(self.s, int(scan_index), _vp(out[0:1]), _vp(out[1:2])), "msfl_slam_get_rejection")
        return out[0], out[1]

    def get_degeneracy(self, scan_index):
        """(odometry, mapping) records of DEGENERACY_DTYPE of one of the last four scans fed (waits for it)."""
        out = np.zeros(2, DEGENERACY_DTYPE)
        self._check(self.lib.msfl_slam_get_degeneracy(self.s, int(scan_index), _vp(out[0:1]), _vp(out[1:2])), "msfl_slam_get_degeneracy")
        return out[0], out[1]

    def set_next_prior(self, odometry=None, mapping=None):
        """Pose priors for the NEXT add_scan only: each a (pose7, sqrt_information 6 x 6) pair or None.  `odometry` joins that scan's
        scan-to-scan solve (relative pose), `mapping` its scan-to-map solve (world pose)."""
        rec = [None if p is None else pose_priors(p[0], [p[1]]) for p in (odometry, mapping)]
        self._check(self.lib.msfl_slam_set_next_prior(self.s, _vp(rec[0]), _vp(rec[1])), "msfl_slam_set_next_prior")

    def get_uncertainty(self, scan_index):
        """(odometry, mapping) records of one of the last four scans fed: a numpy structured array of two UNCERTAINTY_DTYPE records."""
        out = np.zeros(2, UNCERTAINTY_DTYPE)
        self._check(self.lib.msfl_slam_get_uncertainty(self.s, int(scan_index), _vp(out[0:1]), _vp(out[1:2])), "msfl_slam_get_uncertainty")
        return out

    def set_map_window(self, half_cells, every_n_scans=1):
        """Crop both map stores to +-half_cells cells around pose_map after the inserts of every every_n_scans-th scan fed from
        now on (msfl_slam_set_map_window); half_cells=None turns the window off."""
        half = None if half_cells is None else (C.c_int * 3)(*[int(v) for v in half_cells])
        self._check(self.lib.msfl_slam_set_map_window(self.s, half, int(every_n_scans)), "msfl_slam_set_map_window")

    def get_map_window(self, scan_index):
        """(corner, surf) GridCropInfo of one of the last four scans fed; all zero where no crop ran."""
        a, b = GridCropInfo(), GridCropInfo()
        self._check(self.lib.msfl_slam_get_map_window(self.s, int(scan_index), C.byref(a), C.byref(b)), "msfl_slam_get_map_window")
        return a, b

    def clouds(self, scan_index):
        """keep_clouds=1: the scan's data products as host arrays (msfl_slam_get_clouds, MSFL_MEM_HOST): dict with full_scan (n,4),
        full_map (n,4), ring (n,), sharp / less_sharp / flat / less_flat index arrays.  Only for one of the last two scans fed."""
        n = self.max_scan_points
        full_scan, full_map = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        ring = np.zeros(n, np.uint16)
        idx = [np.zeros(n, np.int32) for _ in range(4)]
        c = SlamClouds()
        c.full_scan, c.full_map, c.ring = full_scan.ctypes.data, full_map.ctypes.data, ring.ctypes.data
        c.sharp_idx, c.less_sharp_idx, c.flat_idx, c.less_flat_idx = (a.ctypes.data for a in idx)
        self._check(self.lib.msfl_slam_get_clouds(self.s, int(scan_index), C.byref(c), MEM_HOST), "msfl_slam_get_clouds")
        return dict(full_scan=full_scan[:c.n_full], full_map=full_map[:c.n_full], ring=ring[:c.n_full], sharp=idx[0][:c.n_sharp],
                    less_sharp=idx[1][:c.n_less_sharp], flat=idx[2][:c.n_flat], less_flat=idx[3][:c.n_less_flat])

    def grids(self):
        a, b = C.c_void_p(), C.c_void_p()
        self._check(self.lib.msfl_slam_grids(self.s, C.byref(a), C.byref(b)), "msfl_slam_grids")
        res, leaf_c, leaf_s = self._grid_shape
        return _BorrowedGrid(self.lib, a, self.last_error, res, leaf_c), _BorrowedGrid(self.lib, b, self.last_error, res, leaf_s)


class Places(_Owner):
    """Owns one msfl_places: a device-resident database of polar scan descriptors (msfl_places_*), independent of any Handle.
    Keyword arguments are the fields of msfl_place_config (n_ring, n_sector, min_range, max_range, height_offset, capacity)."""
    _PTR, _DESTROY, _ERROR = "p", "msfl_places_destroy", "msfl_places_last_error"

    def __init__(self, device=0, **cfg):
        ref = self._own(load())
        self.config = PlaceConfig()
        self.lib.msfl_places_default_config(C.byref(self.config))
        for k, v in cfg.items():
            if k not in dict(PlaceConfig._fields_):
                raise TypeError("unknown msfl_place_config field %r" % (k,))
            setattr(self.config, k, v)
        s = self.lib.msfl_places_create(C.byref(self.config), device, ref)
        if s != OK:
            raise MsflError(s, "msfl_places_create", "(a config outside its limits, or no GPU: there is no CPU fallback)")

    n_ring = property(lambda self: self.config.n_ring)
    n_sector = property(lambda self: self.config.n_sector)

    def set_stream(self, stream_ptr):
        self._check(self.lib.msfl_places_set_stream(self.p, stream_ptr), "msfl_places_set_stream")

    def synchronize(self):
        self._check(self.lib.msfl_places_synchronize(self.p), "msfl_places_synchronize")

    def size(self):
        return int(self.lib.msfl_places_size(self.p))

    def __len__(self):
        return self.size()

    @staticmethod
    def _scans(scans, off):
        """one (n, 4) cloud, a list of clouds, or concatenated points + offsets -> (points, int32 offsets)"""
        if off is None:
            if isinstance(scans, np.ndarray) and scans.ndim == 2:
                scans = [scans]
            scans = [_pts(a) for a in scans]
            off = np.zeros(len(scans) + 1, np.int32)
            if scans:
                off[1:] = np.cumsum([len(a) for a in scans])
            pts = np.concatenate(scans) if scans else np.zeros((0, 4), np.float32)
            return np.ascontiguousarray(pts, np.float32), off
        return _pts(scans), np.ascontiguousarray(off, np.int32)

    def add(self, scans, off=None, allow=()):
        """Describes and appends scans: one (n, 4) cloud, a list of clouds, or concatenated points with prefix offsets.  Returns the
        index of the first new entry (or the refusing status when it is in `allow`)."""
        pts, off = self._scans(scans, off)
        first = C.c_int(-1)
        s = self._check(self.lib.msfl_places_add(self.p, _vp(pts), _vp(off), len(off) - 1, MEM_HOST, C.byref(first)), "msfl_places_add", allow)
        return first.value if s == OK else s

    def add_device(self, pts, off, allow=()):
        """Device-pointer form (torch tensor / raw pointer of 16-byte points), asynchronous on the object's stream; `off` is a host array."""
        off = np.ascontiguousarray(off, np.int32)
        first = C.c_int(-1)
        s = self._check(self.lib.msfl_places_add(self.p, _vp(pts), _vp(off), len(off) - 1, MEM_DEVICE, C.byref(first)), "msfl_places_add(device)",
                        allow)
        return first.value if s == OK else s

    def _desc(self, desc):
        d = np.ascontiguousarray(np.asarray(desc, np.float32).reshape(-1, self.n_ring, self.n_sector))
        return d

    def add_descriptors(self, desc, allow=()):
        """Appends ready descriptors (n, n_ring, n_sector) float32 - what get() delivered; keys and norms are recomputed."""
        d = self._desc(desc)
        first = C.c_int(-1)
        s = self._check(self.lib.msfl_places_add_descriptors(self.p, _vp(d), len(d), MEM_HOST, C.byref(first)), "msfl_places_add_descriptors", allow)
        return first.value if s == OK else s

    def add_descriptors_device(self, desc, n, allow=()):
        first = C.c_int(-1)
        s = self._check(self.lib.msfl_places_add_descriptors(self.p, _vp(desc), int(n), MEM_DEVICE, C.byref(first)),
                        "msfl_places_add_descriptors(device)", allow)
        return first.value if s == OK else s

    def get(self, first=0, n=None, want_ring_key=False):
        """Descriptors [first, first + n) as (n, n_ring, n_sector) float32; with want_ring_key also the (n, n_ring) int32 ring keys."""
        n = self.size() - first if n is None else int(n)
        d = np.zeros((max(n, 0), self.n_ring, self.n_sector), np.float32)
        rk = np.zeros((max(n, 0), self.n_ring), np.int32) if want_ring_key else None
        self._check(self.lib.msfl_places_get(self.p, int(first), n, _vp(d), _vp(rk), MEM_HOST), "msfl_places_get")
        return (d, rk) if want_ring_key else d

    def get_device(self, first, n, desc_out, ring_key_out=None):
        self._check(self.lib.msfl_places_get(self.p, int(first), int(n), _vp(desc_out), _vp(ring_key_out), MEM_DEVICE), "msfl_places_get(device)")

    @staticmethod
    def _max_index(max_index, n):
        if max_index is None:
            return None
        m = np.ascontiguousarray(np.broadcast_to(np.asarray(max_index, np.int32), (n,)))
        return m

    def query(self, scans, off=None, max_index=None, n_prefilter=0, k=1, allow=()):
        """The k best entries for each scan: (Q, k) records of PLACE_MATCH_DTYPE ordered by (distance, index).  max_index: None (every
        entry), one int or one per query: only entries below it are candidates."""
        pts, off = self._scans(scans, off)
        Q = len(off) - 1
        out = np.zeros((max(Q, 0), max(int(k), 0)), PLACE_MATCH_DTYPE)
        mi = self._max_index(max_index, Q)
        s = self._check(self.lib.msfl_places_query(self.p, _vp(pts), _vp(off), Q, _vp(mi), int(n_prefilter), int(k), _vp(out), MEM_HOST),
                        "msfl_places_query", allow)
        return out if s == OK else s

    def query_device(self, pts, off, out, max_index=None, n_prefilter=0, k=1, allow=()):
        """Device-pointer form, asynchronous: `out` holds Q x k records of 24 bytes on the device; off / max_index are host arrays."""
        off = np.ascontiguousarray(off, np.int32)
        mi = self._max_index(max_index, len(off) - 1)
        return self._check(self.lib.msfl_places_query(self.p, _vp(pts), _vp(off), len(off) - 1, _vp(mi), int(n_prefilter), int(k), _vp(out),
                                                      MEM_DEVICE), "msfl_places_query(device)", allow)

    def query_entries(self, entries, max_index=None, n_prefilter=0, k=1, allow=()):
        """As query(), for entries that are stored already (e.g. entry i against max_index = i - 50: the loop-closure search)."""
        e = np.ascontiguousarray(np.atleast_1d(np.asarray(entries, np.int32)))
        out = np.zeros((len(e), max(int(k), 0)), PLACE_MATCH_DTYPE)
        mi = self._max_index(max_index, len(e))
        s = self._check(self.lib.msfl_places_query_entries(self.p, _vp(e), len(e), _vp(mi), int(n_prefilter), int(k), _vp(out), MEM_HOST),
                        "msfl_places_query_entries", allow)
        return out if s == OK else s

    def query_entries_device(self, entries, out, max_index=None, n_prefilter=0, k=1, allow=()):
        e = np.ascontiguousarray(np.atleast_1d(np.asarray(entries, np.int32)))
        mi = self._max_index(max_index, len(e))
        return self._check(self.lib.msfl_places_query_entries(self.p, _vp(e), len(e), _vp(mi), int(n_prefilter), int(k), _vp(out), MEM_DEVICE),
                           "msfl_places_query_entries(device)", allow)


class GraphConfig(C.Structure):
    """msfl_graph_config: capacities and the options of the trust-region solve and of its CG step solver."""
    _fields_ = [("max_nodes", C.c_int), ("max_edges", C.c_int), ("max_fixes", C.c_int), ("max_num_iterations", C.c_int),
                ("max_consecutive_invalid_steps", C.c_int), ("jacobi_scaling", C.c_int), ("max_cg_iterations", C.c_int), ("reserved", C.c_int),
                ("huber_delta", C.c_double), ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double),
                ("min_trust_region_radius", C.c_double), ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double),
                ("max_lm_diagonal", C.c_double), ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double), ("cg_tolerance", C.c_double)]


class GraphSummary(C.Structure):
    """msfl_graph_summary: how the last msfl_graph_optimize ended."""
    _fields_ = [("status", C.c_int), ("termination", C.c_int), ("iterations", C.c_int), ("successful_steps", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("cg_iterations", C.c_int), ("cg_unconverged", C.c_int),
                ("n_long_edges", C.c_int), ("n_free", C.c_int)]


# msfl_graph_edge / msfl_graph_fix as numpy structured dtypes (PoseGraph.add_edges, PoseGraph.add_fixes)
GRAPH_EDGE_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("z", np.float64, (7,)), ("sr", np.float64), ("st", np.float64)])
GRAPH_FIX_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("t", np.float64), ("p", np.float64, (3,)), ("st", np.float64)])
assert GRAPH_EDGE_DTYPE.itemsize == 80 and GRAPH_FIX_DTYPE.itemsize == 48 and C.sizeof(GraphSummary) == 48

# msfl_graph_edge_info / msfl_graph_fix_info: the same factors with a full square-root information matrix (row-major)
GRAPH_EDGE_INFO_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("z", np.float64, (7,)), ("sqrt_information", np.float64, (6, 6))])
GRAPH_FIX_INFO_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("t", np.float64), ("p", np.float64, (3,)), ("sqrt_information", np.float64, (3, 3))])
assert GRAPH_EDGE_INFO_DTYPE.itemsize == 352 and GRAPH_FIX_INFO_DTYPE.itemsize == 112
GRAPH_FACTOR_EDGE, GRAPH_FACTOR_FIX, GRAPH_FACTOR_EDGE_INFO, GRAPH_FACTOR_FIX_INFO = range(4)
# msfl_graph_loss: the loss of one factor (PoseGraph.set_losses); `a` is read by HUBER and the kinds after it
GRAPH_LOSS_DEFAULT, GRAPH_LOSS_NONE, GRAPH_LOSS_HUBER, GRAPH_LOSS_SOFT_L_ONE, GRAPH_LOSS_CAUCHY, GRAPH_LOSS_GEMAN_MCCLURE = range(6)
GRAPH_LOSS_NAMES = ("default", "none", "huber", "soft_l_one", "cauchy", "geman_mcclure")
GRAPH_LOSS_DTYPE = np.dtype([("kind", np.int32), ("reserved", np.int32), ("a", np.float64)])
assert GRAPH_LOSS_DTYPE.itemsize == 16

GRAPH_TERMINATION = ("empty", "gradient", "max_iterations", "min_radius", "invalid_steps", "parameter", "function")


class GraphMarginalsSummary(C.Structure):
    """msfl_graph_marginals_summary: how one msfl_graph_marginals call went."""
    _fields_ = [("n_pairs", C.c_int), ("n_columns", C.c_int), ("cg_iterations", C.c_int), ("cg_unconverged", C.c_int),
                ("singular", C.c_int), ("pad", C.c_int), ("min_pivot_ratio", C.c_double)]


class GraphMarginalsOptions(C.Structure):
    """msfl_graph_marginals_options: the pivot test's threshold, the CG cap per column and the byte budget of the column blocks."""
    _fields_ = [("min_pivot_ratio", C.c_double), ("max_cg_iterations", C.c_int), ("reserved", C.c_int), ("scratch_bytes", C.c_ulonglong)]


assert C.sizeof(GraphMarginalsSummary) == 32 and C.sizeof(GraphMarginalsOptions) == 24


def relative_covariance(pose_a, pose_b, S_aa, S_ab, S_bb, out=None):
    """msfl_graph_relative_covariance: the 6 x 6 covariance of T_a^-1 T_b in an information edge's tangent from the joint marginal
    PoseGraph.marginals delivers.  Host arithmetic only.  Returns (status, block); a refusal leaves the block (`out`) untouched."""
    lib = load()
    res = np.zeros((6, 6), np.float64) if out is None else out
    pa, pb = (np.ascontiguousarray(np.asarray(p, np.float64).reshape(7)) for p in (pose_a, pose_b))
    S = [np.ascontiguousarray(np.asarray(m, np.float64).reshape(36)) for m in (S_aa, S_ab, S_bb)]
    s = lib.msfl_graph_relative_covariance(_vp(pa), _vp(pb), _vp(S[0]), _vp(S[1]), _vp(S[2]), _vp(res))
    return int(s), res


def relative_pose(Ti, Tj):
    """T_i^-1 T_j of two poses [t, qx qy qz qw] (unit quaternions): the measurement z of a graph edge (i, j)."""
    Ti, Tj = np.asarray(Ti, np.float64), np.asarray(Tj, np.float64)

    def rot(q, v):
        u, w = q[:3], q[3]
        uv = np.cross(u, v)
        return v + 2.0 * (w * uv + np.cross(u, uv))

    qi = np.array([-Ti[3], -Ti[4], -Ti[5], Ti[6]])
    qj = Tj[3:]
    q = np.concatenate([qi[3] * qj[:3] + qj[3] * qi[:3] + np.cross(qi[:3], qj[:3]), [qi[3] * qj[3] - qi[:3] @ qj[:3]]])
    return np.concatenate([rot(qi, Tj[:3] - Ti[:3]), q])


def edge_from_uncertainty(i, j, pose_i, pose_j, unc, scale, out=None):
    """msfl_graph_edge_from_uncertainty: the information edge (one record of GRAPH_EDGE_INFO_DTYPE) a registration gives.  pose_j is the
    registered pose, `unc` its record (a MatchUncertainty or one element of UNCERTAINTY_DTYPE), `scale` the variance factor (unc's
    sigma2, or a sensor model's).  Host arithmetic only.  Returns (status, record); a refusal leaves the record (`out`) untouched."""
    lib = load()
    rec = np.zeros(1, GRAPH_EDGE_INFO_DTYPE) if out is None else out
    if not isinstance(unc, MatchUncertainty):
        u = np.ascontiguousarray(np.asarray(unc, UNCERTAINTY_DTYPE).reshape(1))
        unc = MatchUncertainty.from_buffer_copy(u.tobytes())
    pi, pj = (np.ascontiguousarray(np.asarray(p, np.float64).reshape(7)) for p in (pose_i, pose_j))
    s = lib.msfl_graph_edge_from_uncertainty(int(i), int(j), _vp(pi), _vp(pj), C.byref(unc), scale, _vp(rec))
    return int(s), rec


def fix_from_covariance(i, j, t, p, covariance, out=None):
    """msfl_graph_fix_from_covariance: the information fix (one record of GRAPH_FIX_INFO_DTYPE) of a position with a 3 x 3 covariance.
    Returns (status, record); a refusal leaves the record (`out`) untouched."""
    lib = load()
    rec = np.zeros(1, GRAPH_FIX_INFO_DTYPE) if out is None else out
    pp = np.ascontiguousarray(np.asarray(p, np.float64).reshape(3))
    cov = np.ascontiguousarray(np.asarray(covariance, np.float64).reshape(9))
    s = lib.msfl_graph_fix_from_covariance(int(i), int(j), t, _vp(pp), _vp(cov), _vp(rec))
    return int(s), rec


class PoseGraph(_Owner):
    """Owns one msfl_graph: poses on the device, relative-pose edges and position fixes, and the trust-region solve over them
    (msfl_graph_*), independent of any Handle.  Keyword arguments are the fields of msfl_graph_config."""
    _PTR, _DESTROY, _ERROR = "p", "msfl_graph_destroy", "msfl_graph_last_error"

    def __init__(self, device=0, **cfg):
        ref = self._own(load())
        self.config = GraphConfig()
        self.lib.msfl_graph_default_config(C.byref(self.config))
        for k, v in cfg.items():
            if k not in dict(GraphConfig._fields_):
                raise TypeError("unknown msfl_graph_config field %r" % (k,))
            setattr(self.config, k, v)
        self._count = [0, 0, 0, 0]               # factors per kind (GRAPH_FACTOR_*), for chi2's default range
        s = self.lib.msfl_graph_create(C.byref(self.config), device, ref)
        if s != OK:
            raise MsflError(s, "msfl_graph_create", "(a config outside its limits, or no GPU: there is no CPU fallback)")

    def set_stream(self, stream_ptr):
        self._check(self.lib.msfl_graph_set_stream(self.p, stream_ptr), "msfl_graph_set_stream")

    def synchronize(self):
        self._check(self.lib.msfl_graph_synchronize(self.p), "msfl_graph_synchronize")

    def clear(self):
        self._check(self.lib.msfl_graph_clear(self.p), "msfl_graph_clear")
        self._count = [0, 0, 0, 0]

    def num_nodes(self):
        return int(self.lib.msfl_graph_num_nodes(self.p))

    def __len__(self):
        return self.num_nodes()

    def add_nodes(self, poses, allow=()):
        """Appends poses: an (n, 7) array, or a CUDA tensor of n x 7 float64 (read in place).  Returns the index of the first new node
        (or the refusing status when it is in `allow`)."""
        first = C.c_int(-1)
        if _on_device(poses):
            n, ptr, mem = int(poses.numel() // 7), poses.data_ptr(), MEM_DEVICE
        else:
            poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 7))
            n, ptr, mem = len(poses), _vp(poses), MEM_HOST
        s = self._check(self.lib.msfl_graph_add_nodes(self.p, ptr, n, mem, C.byref(first)), "msfl_graph_add_nodes", allow)
        return first.value if s == OK else s

    @staticmethod
    def edges(i, j, z, sr=0.01, st=0.1):
        """Records of GRAPH_EDGE_DTYPE from index arrays, (n, 7) measurements and scalar or per-edge sr / st."""
        i = np.atleast_1d(np.asarray(i, np.int32))
        rec = np.zeros(len(i), GRAPH_EDGE_DTYPE)
        rec["i"], rec["j"], rec["z"], rec["sr"], rec["st"] = i, j, np.asarray(z, np.float64).reshape(len(i), 7), sr, st
        return rec

    @staticmethod
    def fixes(i, j, t, p, st=0.01):
        """Records of GRAPH_FIX_DTYPE."""
        i = np.atleast_1d(np.asarray(i, np.int32))
        rec = np.zeros(len(i), GRAPH_FIX_DTYPE)
        rec["i"], rec["j"], rec["t"], rec["p"], rec["st"] = i, j, t, np.asarray(p, np.float64).reshape(len(i), 3), st
        return rec

    @staticmethod
    def edges_info(i, j, z, sqrt_information):
        """Records of GRAPH_EDGE_INFO_DTYPE from index arrays, (n, 7) measurements and (n, 6, 6) (or one 6 x 6) square-root information."""
        i = np.atleast_1d(np.asarray(i, np.int32))
        rec = np.zeros(len(i), GRAPH_EDGE_INFO_DTYPE)
        rec["i"], rec["j"], rec["z"] = i, j, np.asarray(z, np.float64).reshape(len(i), 7)
        rec["sqrt_information"] = np.broadcast_to(np.asarray(sqrt_information, np.float64), (len(i), 6, 6))
        return rec

    @staticmethod
    def fixes_info(i, j, t, p, sqrt_information):
        """Records of GRAPH_FIX_INFO_DTYPE."""
        i = np.atleast_1d(np.asarray(i, np.int32))
        rec = np.zeros(len(i), GRAPH_FIX_INFO_DTYPE)
        rec["i"], rec["j"], rec["t"], rec["p"] = i, j, t, np.asarray(p, np.float64).reshape(len(i), 3)
        rec["sqrt_information"] = np.broadcast_to(np.asarray(sqrt_information, np.float64), (len(i), 3, 3))
        return rec

    def add_edges_info(self, rec, allow=()):
        rec = np.ascontiguousarray(rec, GRAPH_EDGE_INFO_DTYPE)
        s = self._check(self.lib.msfl_graph_add_edges_info(self.p, _vp(rec), len(rec)), "msfl_graph_add_edges_info", allow)
        if s == OK:
            self._count[GRAPH_FACTOR_EDGE_INFO] += len(rec)
        return s

    def add_fixes_info(self, rec, allow=()):
        rec = np.ascontiguousarray(rec, GRAPH_FIX_INFO_DTYPE)
        s = self._check(self.lib.msfl_graph_add_fixes_info(self.p, _vp(rec), len(rec)), "msfl_graph_add_fixes_info", allow)
        if s == OK:
            self._count[GRAPH_FACTOR_FIX_INFO] += len(rec)
        return s

    def chi2(self, kind, first=0, n=None, allow=()):
        """|r|^2 of factors first .. first + n (default: to the last) of one kind (GRAPH_FACTOR_*) at the current poses, before the loss."""
        if n is None:
            n = self._count[int(kind)] - int(first)
        out = np.zeros(max(0, int(n)), np.float64)
        s = self._check(self.lib.msfl_graph_factor_chi2(self.p, int(kind), int(first), int(n), _vp(out)), "msfl_graph_factor_chi2", allow)
        return out if s == OK else s

    @staticmethod
    def loss_records(kind, a=0.0):
        """Records of GRAPH_LOSS_DTYPE from loss kinds (GRAPH_LOSS_*) and their parameters, scalars or arrays."""
        kind = np.atleast_1d(np.asarray(kind, np.int32))
        rec = np.zeros(len(kind), GRAPH_LOSS_DTYPE)
        rec["kind"], rec["a"] = kind, a
        return rec

    def set_losses(self, factor_kind, rec, first=0, n=None, allow=()):
        """msfl_graph_set_losses: gives factors first .. first + n (default: to the last) of one kind (GRAPH_FACTOR_*) the records `rec`
        (GRAPH_LOSS_DTYPE, or a (loss kind, a) pair): n of them, or one for all."""
        if isinstance(rec, tuple):
            rec = self.loss_records(*rec)
        rec = np.ascontiguousarray(rec, GRAPH_LOSS_DTYPE)
        if n is None:
            n = self._count[int(factor_kind)] - int(first) if 0 <= int(factor_kind) < 4 else len(rec)
        return self._check(self.lib.msfl_graph_set_losses(self.p, int(factor_kind), int(first), int(n), _vp(rec), len(rec)), "msfl_graph_set_losses",
                           allow)

    def losses(self, factor_kind, first=0, n=None, allow=()):
        """msfl_graph_get_losses: the records (GRAPH_LOSS_DTYPE) of factors first .. first + n of one kind; DEFAULT where none was set."""
        if n is None:
            n = self._count[int(factor_kind)] - int(first)
        out = np.zeros(max(0, int(n)), GRAPH_LOSS_DTYPE)
        s = self._check(self.lib.msfl_graph_get_losses(self.p, int(factor_kind), int(first), int(n), _vp(out)), "msfl_graph_get_losses", allow)
        return out if s == OK else s

    def weights(self, factor_kind, first=0, n=None, allow=()):
        """msfl_graph_factor_weights: rho'(|r|^2) of factors first .. first + n of one kind at the current poses, each under its own loss."""
        if n is None:
            n = self._count[int(factor_kind)] - int(first)
        out = np.zeros(max(0, int(n)), np.float64)
        s = self._check(self.lib.msfl_graph_factor_weights(self.p, int(factor_kind), int(first), int(n), _vp(out)), "msfl_graph_factor_weights",
                        allow)
        return out if s == OK else s

    def marginals(self, pairs, out=None, allow=(), **options):
        """msfl_graph_marginals: the 6 x 6 covariance blocks Sigma_ab of the node pairs (a, b) at the current poses, in [dt ; dtheta]
        (world frame, left rotation vector).  Returns ((n, 6, 6) array, GraphMarginalsSummary); `out`: a CUDA float64 tensor of n x 36
        to fill on the device instead (asynchronous).  Keyword arguments are the fields of msfl_graph_marginals_options.  A refusing
        status that is in `allow` is returned alone."""
        pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        n = len(pairs)
        opt = GraphMarginalsOptions()
        self.lib.msfl_graph_marginals_default_options(C.byref(opt))
        for k, v in options.items():
            if k not in dict(GraphMarginalsOptions._fields_):
                raise TypeError("unknown msfl_graph_marginals_options field %r" % (k,))
            setattr(opt, k, v)
        sm = GraphMarginalsSummary()
        if out is not None and _on_device(out):
            ptr, mem, res = out.data_ptr(), MEM_DEVICE, out
        else:
            res = np.zeros((n, 6, 6), np.float64) if out is None else out      # a C-contiguous float64 array of n x 36 values
            ptr, mem = _vp(res), MEM_HOST
        call = self.lib.msfl_graph_marginals_with if options else self.lib.msfl_graph_marginals
        args = (self.p, _vp(pairs), n, ptr, mem) + ((C.byref(opt),) if options else ()) + (C.byref(sm),)
        s = self._check(call(*args), "msfl_graph_marginals", allow)
        return (res, sm) if s == OK else s

    def add_edges(self, rec, allow=()):
        rec = np.ascontiguousarray(rec, GRAPH_EDGE_DTYPE)
        s = self._check(self.lib.msfl_graph_add_edges(self.p, _vp(rec), len(rec)), "msfl_graph_add_edges", allow)
        if s == OK:
            self._count[GRAPH_FACTOR_EDGE] += len(rec)
        return s

    def add_fixes(self, rec, allow=()):
        rec = np.ascontiguousarray(rec, GRAPH_FIX_DTYPE)
        s = self._check(self.lib.msfl_graph_add_fixes(self.p, _vp(rec), len(rec)), "msfl_graph_add_fixes", allow)
        if s == OK:
            self._count[GRAPH_FACTOR_FIX] += len(rec)
        return s

    def set_fixed(self, node, flag=True, allow=()):
        return self._check(self.lib.msfl_graph_set_fixed(self.p, int(node), 1 if flag else 0), "msfl_graph_set_fixed", allow)

    def set_poses(self, poses, first=0, allow=()):
        if _on_device(poses):
            n, ptr, mem = int(poses.numel() // 7), poses.data_ptr(), MEM_DEVICE
        else:
            poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 7))
            n, ptr, mem = len(poses), _vp(poses), MEM_HOST
        return self._check(self.lib.msfl_graph_set_poses(self.p, int(first), n, ptr, mem), "msfl_graph_set_poses", allow)

    def poses(self, first=0, n=None, out=None):
        """(n, 7) poses from node `first` on; `out`: a CUDA float64 tensor to fill on the device instead (asynchronous)."""
        n = self.num_nodes() - int(first) if n is None else int(n)
        if out is not None:
            self._check(self.lib.msfl_graph_get_poses(self.p, int(first), n, out.data_ptr(), MEM_DEVICE), "msfl_graph_get_poses(device)")
            return out
        a = np.zeros((n, 7), np.float64)
        self._check(self.lib.msfl_graph_get_poses(self.p, int(first), n, _vp(a), MEM_HOST), "msfl_graph_get_poses")
        return a

    def cost(self):
        c = C.c_double(0.0)
        self._check(self.lib.msfl_graph_cost(self.p, C.byref(c)), "msfl_graph_cost")
        return c.value

    def optimize(self):
        """Runs the solve; returns the GraphSummary (termination as a code: GRAPH_TERMINATION names it)."""
        s = GraphSummary()
        self._check(self.lib.msfl_graph_optimize(self.p, C.byref(s)), "msfl_graph_optimize")
        return s

    def trace(self):
        """(accept list, candidate costs) of the last optimize, one entry per LM iteration."""
        cap = max(1, int(self.config.max_num_iterations))
        acc, cost, n = np.zeros(cap, np.int32), np.zeros(cap, np.float64), C.c_int(0)
        self._check(self.lib.msfl_graph_get_trace(self.p, _vp(acc), _vp(cost), cap, C.byref(n)), "msfl_graph_get_trace")
        return acc[:n.value].copy(), cost[:n.value].copy()
