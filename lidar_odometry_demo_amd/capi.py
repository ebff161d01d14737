"""ctypes binding of liblidar_odometry_amd.so (include/lidar_odometry_amd.h).

There is no fallback: if the HIP library is missing this module raises, and
without a gfx950 device every map constructor fails with LOM_ERR_NO_DEVICE.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LOM_LIB_PATH") or os.path.join(_HERE, "liblidar_odometry_amd.so")  # LOM_LIB_PATH: A/B builds (tools/)
NSUMS = 32
COMM_ID_BYTES = 128

OK, ERR_ARG, ERR_OOM, ERR_RANGE, ERR_HIP, ERR_NO_DEVICE, ERR_COMM, ERR_STATE, ERR_HOOK = (
    0, -1, -2, -3, -4, -5, -6, -7, -8)
_ERR_NAMES = {ERR_ARG: "LOM_ERR_ARG", ERR_OOM: "LOM_ERR_OOM", ERR_RANGE: "LOM_ERR_RANGE",
              ERR_HIP: "LOM_ERR_HIP", ERR_NO_DEVICE: "LOM_ERR_NO_DEVICE", ERR_COMM: "LOM_ERR_COMM",
              ERR_STATE: "LOM_ERR_STATE", ERR_HOOK: "LOM_ERR_HOOK"}

EXPORT_FULL, EXPORT_FULL_NO_NORMALS, EXPORT_FIRST_PER_VOXEL = 0, 1, 2


class LomError(RuntimeError):
    def __init__(self, code, text=""):
        self.code = code
        super().__init__(f"{_ERR_NAMES.get(code, code)}: {text}")


class Pose(C.Structure):
    _fields_ = [("t", C.c_float * 3), ("q", C.c_float * 4)]


class Correspondence(C.Structure):
    _fields_ = [("index", C.c_int64), ("origin", C.c_float * 3), ("normal", C.c_float * 3),
                ("sq_dist", C.c_float), ("n_cand", C.c_uint32), ("n_occ", C.c_uint32)]


CORR_DTYPE = np.dtype(
    [("index", "<i8"), ("origin", "<f4", 3), ("normal", "<f4", 3), ("sq_dist", "<f4"),
     ("n_cand", "<u4"), ("n_occ", "<u4")], align=True)


class AlignStats(C.Structure):
    _fields_ = [
        ("outer_iterations", C.c_int32), ("lm_iterations", C.c_int32), ("evaluations", C.c_int32),
        ("match_launches", C.c_int32), ("queries", C.c_int64), ("valid_last", C.c_int64),
        ("cand_total", C.c_int64), ("occ_total", C.c_int64), ("final_cost", C.c_double),
        ("last_step_norm", C.c_double), ("match_kernel_ms", C.c_double),
        ("algorithmic_bytes", C.c_double), ("host_launch_ms", C.c_double), ("host_wait_ms", C.c_double),
        ("profiled_launches", C.c_int64), ("host_fallback", C.c_int32), ("lm_workgroups", C.c_int32),
        ("lm_kernel_ms", C.c_double), ("lm_profiled_launches", C.c_int64),
    ]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AlignProblem(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("n", C.c_size_t), ("stride_bytes", C.c_size_t), ("guess_t", C.c_float * 3),
                ("guess_q_wxyz", C.c_float * 4)]


class AlignMultiProblem(C.Structure):
    _fields_ = [("map", C.c_void_p), ("xyz", C.c_void_p), ("n", C.c_size_t), ("stride_bytes", C.c_size_t),
                ("guess_t", C.c_float * 3), ("guess_q_wxyz", C.c_float * 4)]


class AlignResult(C.Structure):
    _fields_ = [("t", C.c_float * 3), ("q_wxyz", C.c_float * 4), ("stats", AlignStats), ("round", C.c_int32),
                ("pad", C.c_int32)]


NQSUMS = 36


class QualityReport(C.Structure):
    """lom_quality_report"""
    _fields_ = [("queries", C.c_int64), ("valid", C.c_int64), ("inliers", C.c_int64), ("overlap", C.c_double),
                ("cost", C.c_double), ("rmse", C.c_double), ("rmse_inliers", C.c_double),
                ("max_abs_residual", C.c_double), ("mean_sq_dist", C.c_double), ("sigma2", C.c_double),
                ("sum_w", C.c_double), ("information", C.c_double * 36), ("gradient", C.c_double * 6),
                ("eig_t", C.c_double * 3), ("eigvec_t", C.c_double * 9), ("eig_r", C.c_double * 3),
                ("eigvec_r", C.c_double * 9), ("covariance", C.c_double * 36), ("degenerate_t", C.c_int32),
                ("degenerate_r", C.c_int32), ("covariance_valid", C.c_int32), ("pad", C.c_int32)]

    _SHAPES = {"information": (6, 6), "covariance": (6, 6), "eigvec_t": (3, 3), "eigvec_r": (3, 3)}

    def asdict(self):
        """Scalars as Python numbers, arrays as numpy (information / covariance 6x6, eigenvectors 3x3 with row k the
        eigenvector of eigenvalue k)."""
        out = {}
        for k, _ in self._fields_:
            if k == "pad":
                continue
            v = getattr(self, k)
            if isinstance(v, C.Array):
                v = np.array(v[:], np.float64)
                if k in self._SHAPES:
                    v = v.reshape(self._SHAPES[k])
            out[k] = v
        return out


class QualityProblem(C.Structure):
    """lom_quality_problem"""
    _fields_ = [("xyz", C.c_void_p), ("n", C.c_size_t), ("stride_bytes", C.c_size_t), ("t", C.c_float * 3),
                ("q_wxyz", C.c_float * 4)]


# lidar_point::PointXYZIRT (src/lidar_point_type.h:13-21), 32 bytes
POINT_XYZIRT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad0", "<f4"), ("intensity", "<f4"),
                         ("ring", "<u2"), ("pad1", "<u2"), ("time", "<f4"), ("pad2", "<f4")])
assert POINT_XYZIRT.itemsize == 32


class OdometryParams(C.Structure):
    _fields_ = [("lidar_min_range", C.c_float), ("lidar_max_range", C.c_float), ("keyframe_voxel_size", C.c_float),
                ("keyframe_max_points_cnt", C.c_uint32), ("keyframe_matching_voxel_size", C.c_float),
                ("keyframe_update_voxel_size", C.c_float), ("keyframe_cleanup_range", C.c_float),
                ("angular_divergence_threshold", C.c_float)]


class OdometryFrameStats(C.Structure):
    _fields_ = [("planar_points", C.c_int64), ("filtered_points", C.c_int64), ("update_points", C.c_int64),
                ("matching_points", C.c_int64), ("keyframe_voxels", C.c_int64), ("queries", C.c_int64),
                ("outer_iterations", C.c_int32), ("initialised_keyframe", C.c_int32),
                ("unstable_rotation", C.c_int32), ("host_stages", C.c_int32), ("queries_total", C.c_int64)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class NeighbourhoodParams(C.Structure):
    """lom_neighbourhood_params (no defaults: every field is the caller's)"""
    _fields_ = [("radius", C.c_float), ("index_cap", C.c_uint32), ("min_neighbours", C.c_uint32),
                ("max_variation", C.c_float), ("min_spread", C.c_float)]


class CarveParams(C.Structure):
    """lom_carve_params (no defaults: every field is the caller's)"""
    _fields_ = [("margin", C.c_float), ("min_range", C.c_float), ("max_range", C.c_float), ("min_crossings", C.c_uint32)]


class CarveStats(C.Structure):
    """lom_carve_stats"""
    _fields_ = [("rays_walked", C.c_uint64), ("rays_skipped", C.c_uint64), ("cells_visited", C.c_uint64),
                ("voxels_crossed", C.c_uint32), ("voxels_protected", C.c_uint32), ("voxels_erased", C.c_uint32)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# lom_neighbourhood_detail, one per input point
NEIGHBOURHOOD_DETAIL = np.dtype([("neighbours", "<u4"), ("planar", "<i4"), ("eig", "<f8", 3)])
assert NEIGHBOURHOOD_DETAIL.itemsize == 32
CLASSIFIER_RINGS, CLASSIFIER_NEIGHBOURHOOD = 0, 1


class PlaceParams(C.Structure):
    """lom_place_params (no defaults: every field is the caller's)"""
    _fields_ = [("rings", C.c_uint32), ("sectors", C.c_uint32), ("max_range", C.c_float), ("z_floor", C.c_float)]


# lom_place_match, one per (query, rank)
PLACE_MATCH = np.dtype([("id", "<i8"), ("distance", "<f4"), ("shift", "<u4")])
assert PLACE_MATCH.itemsize == 16 and C.sizeof(PlaceParams) == 16


class GraphParams(C.Structure):
    """lom_graph_params (no defaults: every field is the caller's)"""
    _fields_ = [("lambda0", C.c_double), ("gtol", C.c_double), ("xtol", C.c_double), ("pcg_rtol", C.c_double),
                ("max_outer", C.c_int32), ("max_pcg", C.c_int32)]


class GraphStats(C.Structure):
    """lom_graph_stats"""
    _fields_ = [("outer", C.c_int32), ("accepted", C.c_int32), ("pcg_total", C.c_int32), ("pcg_capped", C.c_int32),
                ("stop_reason", C.c_int32), ("pad", C.c_int32), ("cost_initial", C.c_double), ("cost_final", C.c_double),
                ("grad_max", C.c_double), ("lambda_final", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


# lom_graph_pose, one per node / measurement
GRAPH_POSE = np.dtype([("t", "<f8", 3), ("q_wxyz", "<f8", 4)])
assert GRAPH_POSE.itemsize == 56 and C.sizeof(GraphParams) == 40 and C.sizeof(GraphStats) == 56
GRAPH_STOP_GRADIENT, GRAPH_STOP_STEP, GRAPH_STOP_MAX_OUTER = 1, 2, 3


class AssembleParams(C.Structure):
    """lom_assemble_params (radius <= 0: keep everything)"""
    _fields_ = [("centre", C.c_float * 3), ("radius", C.c_float)]


class AssembleStats(C.Structure):
    """lom_assemble_stats"""
    _fields_ = [("scans", C.c_int64), ("points_in", C.c_int64), ("points_kept", C.c_int64), ("voxels_before", C.c_int64),
                ("voxels_after", C.c_int64), ("points_stored_after", C.c_int64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(AssembleParams) == 16 and C.sizeof(AssembleStats) == 48


class VoteParams(C.Structure):
    """lom_vote_params (no defaults: every field is the caller's)"""
    _fields_ = [("margin", C.c_float), ("min_range", C.c_float), ("max_range", C.c_float), ("clearance", C.c_float),
                ("min_free_scans", C.c_uint32), ("free_per_seen", C.c_uint32)]


class VoteStats(C.Structure):
    """lom_vote_stats"""
    _fields_ = [("scans", C.c_uint64), ("rays_walked", C.c_uint64), ("rays_skipped", C.c_uint64),
                ("cells_visited", C.c_uint64), ("voxels_free", C.c_uint32), ("voxels_protected", C.c_uint32),
                ("voxels_erased", C.c_uint32)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(VoteParams) == 24 and C.sizeof(VoteStats) == 48


class OccupancyGeometry(C.Structure):
    """lom_occupancy_geometry"""
    _fields_ = [("resolution", C.c_float), ("origin_x", C.c_float), ("origin_y", C.c_float), ("width", C.c_uint32),
                ("height", C.c_uint32)]

    def asdict(self):
        return dict(resolution=float(self.resolution), origin_x=float(self.origin_x), origin_y=float(self.origin_y),
                    width=int(self.width), height=int(self.height))


class OccupancyRayParams(C.Structure):
    """lom_occupancy_ray_params (no defaults: every field is the caller's)"""
    _fields_ = [("z_lo", C.c_float), ("z_hi", C.c_float), ("margin", C.c_float), ("min_range", C.c_float),
                ("max_range", C.c_float)]


class OccupancyRule(C.Structure):
    """lom_occupancy_rule"""
    _fields_ = [("min_free_scans", C.c_uint32), ("free_per_seen", C.c_uint32), ("min_seen_scans", C.c_uint32)]


class OccupancyStats(C.Structure):
    """lom_occupancy_stats"""
    _fields_ = [("scans", C.c_uint64), ("rays_walked", C.c_uint64), ("rays_skipped", C.c_uint64),
                ("endpoints_marked", C.c_uint64), ("cells_visited", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class OccupancySummary(C.Structure):
    """lom_occupancy_summary"""
    _fields_ = [("cells_free", C.c_uint64), ("cells_occupied", C.c_uint64), ("cells_unknown", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(OccupancyGeometry) == 20 and C.sizeof(OccupancyRayParams) == 20 and C.sizeof(OccupancyRule) == 12
assert C.sizeof(OccupancyStats) == 40 and C.sizeof(OccupancySummary) == 24
OCC_FREE, OCC_OCCUPIED, OCC_UNKNOWN = 0, 100, -1
OCC_OPT_TEST_SLICE_MAX, OCC_OPT_TEST_WINDOW = 1, 2


class ElevationGeometry(C.Structure):
    """lom_elevation_geometry"""
    _fields_ = [("resolution", C.c_float), ("origin_x", C.c_float), ("origin_y", C.c_float), ("width", C.c_uint32),
                ("height", C.c_uint32), ("z_ref", C.c_float)]

    def asdict(self):
        return dict(resolution=float(self.resolution), origin_x=float(self.origin_x), origin_y=float(self.origin_y),
                    width=int(self.width), height=int(self.height), z_ref=float(self.z_ref))


class ElevationPointParams(C.Structure):
    """lom_elevation_point_params (no defaults: every field is the caller's)"""
    _fields_ = [("z_lo", C.c_float), ("z_hi", C.c_float), ("min_range", C.c_float), ("max_range", C.c_float)]


class ElevationLayerParams(C.Structure):
    """lom_elevation_layer_params"""
    _fields_ = [("min_points", C.c_uint32), ("window", C.c_uint32)]


class ElevationCostParams(C.Structure):
    """lom_elevation_cost_params"""
    _fields_ = [("max_slope", C.c_float), ("max_step", C.c_float), ("max_rough", C.c_float), ("max_span", C.c_float)]


class ElevationStats(C.Structure):
    """lom_elevation_stats"""
    _fields_ = [("scans", C.c_uint64), ("points", C.c_uint64), ("points_marked", C.c_uint64),
                ("points_out_of_height", C.c_uint64), ("cells_new", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class ElevationSummary(C.Structure):
    """lom_elevation_summary"""
    _fields_ = [("cells_unknown", C.c_uint64), ("cells_lethal", C.c_uint64), ("cells_costed", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(ElevationGeometry) == 24 and C.sizeof(ElevationPointParams) == 16 and C.sizeof(ElevationLayerParams) == 8
assert C.sizeof(ElevationCostParams) == 16 and C.sizeof(ElevationStats) == 40 and C.sizeof(ElevationSummary) == 24
ELEV_QUANTUM_LOG2 = -8
ELEV_COST_UNKNOWN, ELEV_COST_LETHAL = -1, 100
ELEV_OPT_TEST_WAVE_MERGE = 1


class ClearanceParams(C.Structure):
    """lom_clearance_params"""
    _fields_ = [("inflation_radius", C.c_float), ("inscribed_radius", C.c_float), ("decay", C.c_float), ("flags", C.c_uint32)]


class ClearanceWindow(C.Structure):
    """lom_clearance_window"""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32)]


class ClearanceSummary(C.Structure):
    """lom_clearance_summary"""
    _fields_ = [("cells_lethal", C.c_uint64), ("cells_inscribed", C.c_uint64), ("cells_costed", C.c_uint64),
                ("cells_unknown", C.c_uint64), ("cells_invalid", C.c_uint64), ("cells_cleared", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(ClearanceParams) == 16 and C.sizeof(ClearanceWindow) == 16 and C.sizeof(ClearanceSummary) == 48
CLEAR_FAR = 65535
CLEAR_FREE_CLEARS_ELEVATION, CLEAR_UNKNOWN_IS_OBSTACLE = 1, 2
CLEAR_OPT_TEST_TILE_ROWS, CLEAR_OPT_TEST_NO_PRUNE = 1, 2


class NavFieldParams(C.Structure):
    """lom_navfield_params"""
    _fields_ = [("neutral", C.c_uint32), ("factor", C.c_uint32), ("unknown_cost", C.c_uint32), ("max_passable", C.c_int8),
                ("flags", C.c_uint32)]


class NavFieldSummary(C.Structure):
    """lom_navfield_summary"""
    _fields_ = [("cells_blocked", C.c_uint64), ("cells_reached", C.c_uint64), ("cells_unreached", C.c_uint64),
                ("cells_invalid", C.c_uint64), ("goals_used", C.c_uint64), ("goals_rejected", C.c_uint64),
                ("range_exceeded", C.c_uint64), ("max_potential", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class NavFieldSolveStats(C.Structure):
    """lom_navfield_solve_stats"""
    _fields_ = [("launches", C.c_uint64), ("waits", C.c_uint64), ("tiles", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(NavFieldParams) == 20 and C.sizeof(NavFieldSummary) == 64 and C.sizeof(NavFieldSolveStats) == 24
NAV_UNREACHED, NAV_MAX = 0xFFFFFFFF, 0xFFFFFFFE
NAV_UNKNOWN_PASSABLE = 1
NAV_CELLS, NAV_METRES = 0, 1
NAV_OPT_TEST_INNER_CAP, NAV_OPT_TEST_BATCH, NAV_OPT_TEST_ALL_TILES = 1, 2, 3


class RegionsParams(C.Structure):
    """lom_regions_params"""
    _fields_ = [("kind", C.c_int32), ("lo", C.c_int8), ("hi", C.c_int8), ("max_cost", C.c_int8), ("min_cells", C.c_uint32),
                ("rank", C.c_int32), ("flags", C.c_uint32)]


class RegionsSummary(C.Structure):
    """lom_regions_summary"""
    _fields_ = [("cells_member", C.c_uint64), ("regions", C.c_uint64), ("regions_recorded", C.c_uint64),
                ("regions_listed", C.c_uint64), ("largest_cells", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class RegionsExtractStats(C.Structure):
    """lom_regions_extract_stats"""
    _fields_ = [("launches", C.c_uint64), ("waits", C.c_uint64), ("tiles", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# lom_regions_record, 48 bytes
REGIONS_RECORD = np.dtype([("label", "<u4"), ("cells", "<u4"), ("sum_x", "<u8"), ("sum_y", "<u8"), ("min_x", "<u2"), ("min_y", "<u2"),
                           ("max_x", "<u2"), ("max_y", "<u2"), ("centroid_x", "<u2"), ("centroid_y", "<u2"), ("centre_x", "<u2"),
                           ("centre_y", "<u2"), ("entry_x", "<u2"), ("entry_y", "<u2"), ("entry_potential", "<u4")])
assert C.sizeof(RegionsParams) == 20 and C.sizeof(RegionsSummary) == 40 and C.sizeof(RegionsExtractStats) == 24
assert REGIONS_RECORD.itemsize == 48
REGIONS_NONE = 0xFFFFFFFF
REGIONS_BYTES, REGIONS_FRONTIER = 0, 1
REGIONS_NEIGHBOURS_8, REGIONS_EDGE_UNKNOWN, REGIONS_CONNECT_4 = 1, 2, 4
REGIONS_RANK_LABEL, REGIONS_RANK_CELLS, REGIONS_RANK_POTENTIAL = 0, 1, 2
REGIONS_GOAL_CENTRE, REGIONS_GOAL_ENTRY = 0, 1
REGIONS_OPT_MAX_REGIONS, REGIONS_OPT_TEST_TILE_ROWS, REGIONS_OPT_TEST_NO_TILES, REGIONS_OPT_TEST_NO_WAVE_MERGE = 1, 2, 3, 4


class VisibilityParams(C.Structure):
    """lom_visibility_params"""
    _fields_ = [("beams", C.c_uint32), ("range_cells", C.c_uint32), ("block_min", C.c_int32), ("unknown_depth", C.c_uint32),
                ("flags", C.c_uint32)]


class VisibilitySummary(C.Structure):
    """lom_visibility_summary"""
    _fields_ = [("viewpoints", C.c_uint64), ("valid", C.c_uint64), ("unknown_total", C.c_uint64), ("unknown_max", C.c_uint64),
                ("unknown_argmax", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class VisibilitySelectParams(C.Structure):
    """lom_visibility_select_params"""
    _fields_ = [("n", C.c_uint32), ("gain_weight", C.c_uint32), ("cost_shift", C.c_uint32), ("min_gain", C.c_uint32)]


class VisibilityCallStats(C.Structure):
    """lom_visibility_call_stats"""
    _fields_ = [("launches", C.c_uint64), ("waits", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# lom_visibility_record, 32 bytes, and lom_visibility_pick, 16 bytes
VISIBILITY_RECORD = np.dtype([("ix", "<i4"), ("iy", "<i4"), ("valid", "<u4"), ("seen", "<u4"), ("unknown", "<u4"), ("free", "<u4"),
                              ("blocked", "<u4"), ("hits", "<u4")])
VISIBILITY_PICK = np.dtype([("k", "<u4"), ("gain", "<u4"), ("score", "<i8")])
assert C.sizeof(VisibilityParams) == 20 and C.sizeof(VisibilitySummary) == 40 and C.sizeof(VisibilitySelectParams) == 16
assert C.sizeof(VisibilityCallStats) == 16 and VISIBILITY_RECORD.itemsize == 32 and VISIBILITY_PICK.itemsize == 16
VIS_KEEP_WINDOWS, VIS_KEEP_BEAMS = 1, 2
VIS_END_INVALID, VIS_END_EDGE, VIS_END_RANGE, VIS_END_HIT, VIS_END_UNKNOWN, VIS_END_CORNER = 0, 1, 2, 3, 4, 5
VIS_OPT_TEST_NO_LDS, VIS_OPT_TEST_WAVES, VIS_OPT_MAX_WINDOW_BYTES = 1, 2, 3


class RolloutParams(C.Structure):
    """lom_rollout_params"""
    _fields_ = [("segments", C.c_uint32), ("steps_per_segment", C.c_uint32), ("lethal_min", C.c_int32), ("unknown_cost", C.c_int32),
                ("min_steps", C.c_uint32), ("progress_weight", C.c_uint32), ("cost_weight", C.c_uint32),
                ("truncation_weight", C.c_uint32), ("flags", C.c_uint32)]


class RolloutSummary(C.Structure):
    """lom_rollout_summary"""
    _fields_ = [("states", C.c_uint64), ("valid_states", C.c_uint64), ("candidates", C.c_uint64), ("admissible", C.c_uint64),
                ("states_without_pick", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class RolloutCallStats(C.Structure):
    """lom_rollout_call_stats"""
    _fields_ = [("launches", C.c_uint64), ("waits", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# lom_rollout_state, 12 bytes, lom_rollout_record, 32 bytes, and lom_rollout_pick, 16 bytes
ROLLOUT_STATE = np.dtype([("x", "<i4"), ("y", "<i4"), ("a", "<u4")])
ROLLOUT_RECORD = np.dtype([("free_poses", "<u4"), ("reason", "<u4"), ("cost_sum", "<u4"), ("cost_max", "<u4"), ("end_x", "<i4"),
                           ("end_y", "<i4"), ("end_angle", "<u4"), ("end_potential", "<u4")])
ROLLOUT_PICK = np.dtype([("k", "<u4"), ("admissible", "<u4"), ("score", "<i8")])
assert C.sizeof(RolloutParams) == 36 and C.sizeof(RolloutSummary) == 40 and C.sizeof(RolloutCallStats) == 16
assert ROLLOUT_STATE.itemsize == 12 and ROLLOUT_RECORD.itemsize == 32 and ROLLOUT_PICK.itemsize == 16
ROLLOUT_TABLE = 4096
ROLLOUT_KEEP_RECORDS = 1
ROLLOUT_OK, ROLLOUT_UNKNOWN, ROLLOUT_COLLISION, ROLLOUT_EDGE, ROLLOUT_INVALID = 0, 1, 2, 3, 4
ROLLOUT_OPT_TEST_SERIAL, ROLLOUT_OPT_TEST_NO_LDS_PLANE, ROLLOUT_OPT_TEST_WAVES = 1, 2, 3
ROLLOUT_NONE = 0xFFFFFFFF


class Pc2Field(C.Structure):
    _fields_ = [("name", C.c_char_p), ("offset", C.c_uint32), ("datatype", C.c_uint8), ("count", C.c_uint32)]


class Pc2View(C.Structure):
    _fields_ = [("height", C.c_uint32), ("width", C.c_uint32), ("fields", C.POINTER(Pc2Field)), ("n_fields", C.c_uint32),
                ("is_bigendian", C.c_uint8), ("point_step", C.c_uint32), ("row_step", C.c_uint32),
                ("data", C.c_void_p), ("data_bytes", C.c_size_t)]


class PcdInfo(C.Structure):
    _fields_ = [("points", C.c_uint64), ("width", C.c_uint32), ("height", C.c_uint32), ("point_step", C.c_uint32),
                ("has_normals", C.c_int32), ("data_kind", C.c_int32)]


MATCH_EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                            C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))
EVAL_FIXED_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                            C.POINTER(C.c_double))
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int)


class AlignHooks(C.Structure):
    _fields_ = [("user", C.c_void_p), ("match_eval", MATCH_EVAL_FN), ("eval_fixed", EVAL_FIXED_FN),
                ("allreduce", ALLREDUCE_FN)]


# every symbol include/lidar_odometry_amd.h declares
EXPORTED = [
    "lom_abi_version", "lom_device_count", "lom_device_local_cpus", "lom_pose_identity", "lom_pose_compose", "lom_pose_inverse",
    "lom_pose_relative_to", "lom_pose_rotation_matrix", "lom_transform_points", "lom_map_create",
    "lom_map_destroy", "lom_last_error", "lom_map_clear", "lom_map_set_max_points", "lom_map_add_points",
    "lom_map_add_points_device", "lom_map_add_points_device_nowait", "lom_map_status", "lom_map_radius_cleanup", "lom_map_radius_cleanup_after_align", "lom_map_size", "lom_map_point_count",
    "lom_map_export", "lom_voxel_downsample", "lom_voxel_downsample_device", "lom_upload_points",
    "lom_transform_points_device", "lom_map_get_stream", "lom_match_find_pairs", "lom_match_find_pairs_sq", "lom_debug_find_pairs_after", "lom_match_align", "lom_match_align_device", "lom_match_align_repeat", "lom_debug_match_stamps", "lom_debug_eval_sums", "lom_debug_lm_trace", "lom_debug_lm_policy",
    "lom_map_set_profiling", "lom_profile_match", "lom_profile_insert", "lom_map_set_stream", "lom_comm_unique_id", "lom_comm_init",
    "lom_comm_finalize", "lom_comm_host_id", "lom_host_comm_create", "lom_host_comm_allreduce",
    "lom_host_comm_destroy", "lom_host_comm_allgather", "lom_comm_attach_host", "lom_comm_attach_p2p", "lom_align_with_hooks", "lom_point_time_normalize", "lom_transform_non_rigid",
    "lom_range_filter", "lom_cloud_classify", "lom_odometry_default_params", "lom_odometry_create",
    "lom_odometry_destroy", "lom_odometry_process_cloud", "lom_odometry_process_sequence", "lom_odometry_hint_next", "lom_odometry_get_pose", "lom_odometry_get_stats", "lom_odometry_get_temp_cloud", "lom_odometry_debug_set_state",
    "lom_odometry_keyframe", "lom_odometry_last_error", "lom_pcd_read", "lom_pcd_last_error", "lom_estimate_normals", "lom_frontend_create", "lom_frontend_destroy", "lom_frontend_last_error",
    "lom_frontend_process", "lom_frontend_results", "lom_frontend_wait", "lom_frontend_fetch", "lom_frontend_stream", "lom_frontend_stage", "lom_map_set_align_idle_hook", "lom_frontend_done_event", "lom_map_wait_event", "lom_frontend_sequence", "lom_map_status_words", "lom_debug_sinf",
    "lom_voxel_downsample_device_nowait", "lom_map_read_device_words", "lom_map_read_device_words_begin", "lom_map_read_device_words_end",
    "lom_pointcloud2_unpack", "lom_pointcloud2_layout", "lom_pointcloud2_pack_xyz", "lom_pointcloud2_last_error",
    "lom_map_set_option", "lom_map_debug_counter", "lom_odometry_set_option", "lom_odometry_debug_counter",
    "lom_frontend_set_option", "lom_host_comm_set_timeout", "lom_host_comm_abort", "lom_host_comm_last_error",
    "lom_scan_create", "lom_scan_destroy", "lom_scan_last_error", "lom_scan_set_option", "lom_scan_set_stream",
    "lom_scan_get_stream", "lom_scan_create_on_partition", "lom_scan_align", "lom_scan_align_device", "lom_scan_align_repeat", "lom_scan_find_pairs", "lom_scan_find_pairs_sq",
    "lom_match_align_batch", "lom_match_align_batch_device", "lom_scan_align_batch", "lom_scan_align_batch_device",
    "lom_align_batch_best", "lom_match_align_multi", "lom_match_align_multi_device", "lom_odometry_process_batch",
    "lom_quality_from_sums", "lom_match_quality", "lom_match_quality_device", "lom_scan_quality", "lom_scan_quality_device",
    "lom_odometry_set_quality_thresholds", "lom_odometry_get_quality",
    "lom_match_quality_batch_sums", "lom_match_quality_batch_sums_device", "lom_match_quality_batch",
    "lom_match_quality_batch_device", "lom_scan_quality_batch_sums", "lom_scan_quality_batch_sums_device",
    "lom_scan_quality_batch", "lom_scan_quality_batch_device", "lom_quality_batch_best", "lom_pose_lattice",
    "lom_classify_neighbourhood", "lom_frontend_set_classifier", "lom_frontend_debug_counter", "lom_odometry_set_classifier",
    "lom_debug_replayed_iterations", "lom_debug_set_host_replay_fold", "lom_debug_replay_fold_count",
    "lom_place_db_create", "lom_place_db_destroy", "lom_place_db_last_error", "lom_place_db_size", "lom_place_db_clear",
    "lom_place_db_params", "lom_place_db_stream", "lom_place_db_device", "lom_place_db_wait_event", "lom_place_describe",
    "lom_place_describe_device", "lom_place_db_add", "lom_place_db_add_cloud", "lom_place_db_add_cloud_device",
    "lom_place_db_get", "lom_place_db_query", "lom_place_db_query_cloud_device", "lom_place_shift_yaw",
    "lom_odometry_place_descriptor", "lom_frontend_deskewed",
    "lom_map_carve_rays", "lom_map_carve_rays_device", "lom_map_carve_counts", "lom_odometry_set_carve",
    "lom_odometry_get_carve_stats",
    "lom_graph_create", "lom_graph_destroy", "lom_graph_last_error", "lom_graph_clear", "lom_graph_stream", "lom_graph_device",
    "lom_graph_add_node", "lom_graph_add_nodes", "lom_graph_add_edge", "lom_graph_add_edges", "lom_graph_node_count",
    "lom_graph_edge_count", "lom_graph_get_poses", "lom_graph_set_pose", "lom_graph_set_fixed", "lom_graph_optimize",
    "lom_graph_evaluate", "lom_graph_debug_matvec", "lom_graph_edge_chi2", "lom_graph_check_gauge", "lom_graph_lm_policy",
    "lom_graph_information_from_quality", "lom_graph_pose_from_f32", "lom_graph_pose_to_f32",
    "lom_archive_create", "lom_archive_destroy", "lom_archive_last_error", "lom_archive_clear", "lom_archive_stream",
    "lom_archive_device", "lom_archive_wait_event", "lom_archive_add", "lom_archive_add_device", "lom_archive_scan_count",
    "lom_archive_point_count", "lom_archive_scan_size", "lom_archive_get", "lom_map_assemble", "lom_odometry_archive_scan",
    "lom_odometry_rebuild_keyframe",
    "lom_map_carve_scans", "lom_map_scan_votes", "lom_odometry_set_rebuild_votes", "lom_odometry_get_rebuild_vote_stats",
    "lom_odometry_archive_deskewed", "lom_odometry_occupancy_scan",
    "lom_occupancy_create", "lom_occupancy_destroy", "lom_occupancy_last_error", "lom_occupancy_clear",
    "lom_occupancy_get_geometry", "lom_occupancy_stream", "lom_occupancy_device", "lom_occupancy_wait_event",
    "lom_occupancy_set_option", "lom_occupancy_integrate", "lom_occupancy_integrate_cloud",
    "lom_occupancy_integrate_cloud_device", "lom_occupancy_counts", "lom_occupancy_classify", "lom_occupancy_classify_device",
    "lom_odometry_elevation_scan",
    "lom_elevation_create", "lom_elevation_destroy", "lom_elevation_last_error", "lom_elevation_clear",
    "lom_elevation_get_geometry", "lom_elevation_stream", "lom_elevation_device", "lom_elevation_wait_event",
    "lom_elevation_set_option", "lom_elevation_integrate", "lom_elevation_integrate_cloud",
    "lom_elevation_integrate_cloud_device", "lom_elevation_cells", "lom_elevation_layers", "lom_elevation_cost",
    "lom_elevation_cost_device",
    "lom_clearance_create", "lom_clearance_destroy", "lom_clearance_last_error", "lom_clearance_clear",
    "lom_clearance_get_geometry", "lom_clearance_stream", "lom_clearance_device", "lom_clearance_wait_event",
    "lom_clearance_set_option", "lom_clearance_update", "lom_clearance_update_device", "lom_clearance_update_from_grids",
    "lom_clearance_cost", "lom_clearance_cost_device", "lom_clearance_distance_sq", "lom_clearance_distance",
    "lom_clearance_cost_table", "lom_clearance_query",
    "lom_navfield_create", "lom_navfield_destroy", "lom_navfield_last_error", "lom_navfield_clear",
    "lom_navfield_get_geometry", "lom_navfield_stream", "lom_navfield_device", "lom_navfield_wait_event",
    "lom_navfield_set_option", "lom_navfield_solve", "lom_navfield_solve_device", "lom_navfield_solve_from_clearance",
    "lom_navfield_potential", "lom_navfield_potential_device", "lom_navfield_paths", "lom_navfield_query",
    "lom_navfield_cell_costs", "lom_navfield_stats",
    "lom_regions_create", "lom_regions_destroy", "lom_regions_last_error", "lom_regions_clear", "lom_regions_get_geometry",
    "lom_regions_stream", "lom_regions_device", "lom_regions_wait_event", "lom_regions_set_option", "lom_regions_extract",
    "lom_regions_extract_device", "lom_regions_extract_from_grids", "lom_regions_labels", "lom_regions_labels_device",
    "lom_regions_list", "lom_regions_goals", "lom_regions_query", "lom_regions_stats",
    "lom_visibility_create", "lom_visibility_destroy", "lom_visibility_last_error", "lom_visibility_clear",
    "lom_visibility_get_geometry", "lom_visibility_stream", "lom_visibility_device", "lom_visibility_wait_event",
    "lom_visibility_set_option", "lom_visibility_table", "lom_visibility_cast", "lom_visibility_cast_device",
    "lom_visibility_cast_from_occupancy", "lom_visibility_records", "lom_visibility_beams", "lom_visibility_windows_device",
    "lom_visibility_windows",    "lom_visibility_select", "lom_visibility_select_from_navfield", "lom_visibility_stats",
    "lom_rollout_create", "lom_rollout_destroy", "lom_rollout_last_error", "lom_rollout_clear", "lom_rollout_get_geometry",
    "lom_rollout_stream", "lom_rollout_device", "lom_rollout_wait_event", "lom_rollout_set_option", "lom_rollout_evaluate",
    "lom_rollout_evaluate_device", "lom_rollout_evaluate_from_grids", "lom_rollout_records", "lom_rollout_stats",
    "lom_rollout_footprint_rectangle", "lom_rollout_state_from_pose", "lom_rollout_poses",
]
# ... and the one it declares through a function type (the "scan archive and map assembly" section)
EXPORTED_BY_TYPE = ["lom_graph_pose_rotation_matrix"]
# ... and the two of the same section that came with the occupancy grid, declared the same way
EXPORTED_BY_TYPE_POINTS = ["lom_archive_add_points", "lom_archive_add_points_device"]

# lom_option / counters of include/lidar_odometry_amd.h
OPT_HOST_LM, OPT_DEVICE_PATIENCE_TICKS, OPT_DEBUG_LM_STAMPS, OPT_DEBUG_TIMING, OPT_NO_TEMPORAL_BOUND, OPT_COUNT_CANDIDATES = 1, 2, 3, 4, 5, 6
OPT_TEST_GIVE_UP_AT_OUTER, OPT_TEST_GRID_GIVE_UP, OPT_TEST_FORCE_HOST_REDO = 100, 101, 102
OPT_NO_BULK_INSERT, OPT_TEST_BULK_PARTITION_MAX = 7, 106
OPT_TEST_BATCH_ROUND_MAX = 107
OPT_TEST_QUALITY_ROUND_MAX = 108
OPT_TEST_VOTE_SLICE_MAX = 109
OPT_QUALITY_REPORT = 8
OPT_REPLAY_FOLD = 9
OPT_TEST_GRID_GIVE_UP_MATCHING_DS, OPT_TEST_GRID_GIVE_UP_UPDATE_DS, OPT_TEST_GRID_GIVE_UP_KEYFRAME = 103, 104, 105
COUNTER_GRID_REDOS = 0
COUNTER_CLEANUPS_BEHIND_ALIGN = 1
COUNTER_FRAMES_SENT_AHEAD = 2
COUNTER_EMPTY_SLABS = 3

_lib = None


def _share_hip_runtime_with_torch():
    """A PyTorch-ROCm wheel bundles its own libamdhip64.so / libhsa-runtime64.so (same
    SONAME as /opt/rocm's).  Two HSA runtimes in one process cannot both own the GPU
    ("No HIP GPUs are available" in whichever comes second), so when such a wheel is
    installed its copy is loaded first and this library binds to it by SONAME.  torch
    itself is not imported."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return  # torch's runtime is already resident; ours will resolve to it
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    """Loads the HIP library; raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C lidar_odometry_demo_amd/csrc`.  There is no CPU fallback.")
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    fp, dp, pp, vp = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(Pose), C.c_void_p
    L.lom_abi_version.restype = C.c_int
    L.lom_device_count.restype = C.c_int
    L.lom_device_local_cpus.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    L.lom_pose_identity.argtypes = [pp]
    L.lom_pose_compose.argtypes = [pp, pp, pp]
    L.lom_pose_inverse.argtypes = [pp, pp]
    L.lom_pose_relative_to.argtypes = [pp, pp, pp]
    L.lom_pose_rotation_matrix.argtypes = [pp, fp]
    L.lom_transform_points.argtypes = [pp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, C.c_size_t]
    L.lom_map_create.argtypes = [C.c_float, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.lom_map_destroy.argtypes = [vp]
    L.lom_map_destroy.restype = None
    L.lom_last_error.argtypes = [vp]
    L.lom_last_error.restype = C.c_char_p
    L.lom_map_clear.argtypes = [vp, C.c_float]
    L.lom_map_set_max_points.argtypes = [vp, C.c_size_t]
    L.lom_map_add_points.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t]
    L.lom_map_add_points_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t]
    L.lom_map_add_points_device_nowait.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t]
    L.lom_map_status.argtypes = [vp]
    L.lom_map_radius_cleanup.argtypes = [vp, fp, C.c_float]
    L.lom_map_radius_cleanup_after_align.argtypes = [vp, C.c_float]
    L.lom_map_size.argtypes = [vp]
    L.lom_map_size.restype = C.c_int64
    L.lom_map_point_count.argtypes = [vp]
    L.lom_map_point_count.restype = C.c_int64
    L.lom_map_export.argtypes = [vp, C.c_int, vp, vp, C.c_size_t]
    L.lom_map_export.restype = C.c_int64
    L.lom_voxel_downsample.argtypes = [vp, C.c_float, vp, vp, C.c_size_t, C.c_size_t, vp, vp, C.c_size_t]
    L.lom_voxel_downsample.restype = C.c_int64
    L.lom_voxel_downsample_device.argtypes = [vp, C.c_float, vp, vp, C.c_size_t, C.c_size_t, C.POINTER(vp), C.POINTER(vp)]
    L.lom_voxel_downsample_device.restype = C.c_int64
    L.lom_upload_points.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.POINTER(vp), C.POINTER(vp)]
    L.lom_upload_points.restype = C.c_int
    L.lom_transform_points_device.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_size_t, C.POINTER(vp), C.POINTER(vp)]
    L.lom_transform_points_device.restype = C.c_int
    L.lom_map_get_stream.argtypes = [vp]
    L.lom_map_get_stream.restype = vp
    L.lom_match_find_pairs.argtypes = [vp, vp, C.c_size_t, C.c_size_t, fp, fp, C.c_float, vp]
    L.lom_match_find_pairs.restype = C.c_int64
    L.lom_match_find_pairs_sq.argtypes = [vp, vp, C.c_size_t, C.c_size_t, fp, fp, C.c_double, vp]
    L.lom_match_find_pairs_sq.restype = C.c_int64
    L.lom_debug_find_pairs_after.argtypes = [vp, vp, C.c_size_t, C.c_size_t, fp, fp, fp, fp, C.c_float, vp]
    L.lom_debug_find_pairs_after.restype = C.c_int64
    L.lom_match_align.argtypes = [vp, vp, C.c_size_t, C.c_size_t, fp, fp, fp, fp, C.POINTER(AlignStats)]
    L.lom_match_align_device.argtypes = L.lom_match_align.argtypes
    L.lom_debug_match_stamps.argtypes = [vp, vp, C.c_size_t, C.c_size_t, fp, fp, C.c_float, vp, C.c_size_t,
                                         C.POINTER(C.c_uint32)]
    L.lom_match_align_batch.argtypes = [vp, C.POINTER(AlignProblem), C.c_int, C.POINTER(AlignResult), C.POINTER(C.c_int)]
    L.lom_match_align_batch_device.argtypes = L.lom_match_align_batch.argtypes
    L.lom_scan_align_batch.argtypes = L.lom_match_align_batch.argtypes
    L.lom_scan_align_batch_device.argtypes = L.lom_match_align_batch.argtypes
    L.lom_align_batch_best.argtypes = [C.POINTER(AlignResult), C.c_int]
    L.lom_match_align_multi.argtypes = [vp, C.POINTER(AlignMultiProblem), C.c_int, C.POINTER(AlignResult),
                                        C.POINTER(C.c_int)]
    L.lom_match_align_multi_device.argtypes = L.lom_match_align_multi.argtypes
    L.lom_match_align_repeat.argtypes = [vp, vp, C.c_size_t, C.c_size_t, fp, fp, C.c_int, fp, fp, C.POINTER(AlignStats)]
    L.lom_debug_eval_sums.argtypes = [vp, vp, C.c_size_t, C.c_size_t, fp, fp, dp, dp, dp]
    L.lom_debug_lm_trace.argtypes = [vp, vp, C.c_size_t, C.c_size_t, fp, fp, C.c_int, dp, C.POINTER(C.c_int), fp, fp,
                                     C.POINTER(AlignStats)]
    L.lom_debug_lm_policy.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), dp, dp, dp, C.POINTER(C.c_int), dp,
                                      C.POINTER(C.c_int), C.POINTER(C.c_int), dp, dp]
    L.lom_debug_replayed_iterations.argtypes = [vp]
    L.lom_debug_set_host_replay_fold.argtypes = [C.c_int]
    L.lom_debug_replay_fold_count.argtypes = [C.c_int, C.c_double]
    L.lom_map_set_profiling.argtypes = [vp, C.c_int]
    L.lom_map_set_stream.argtypes = [vp, vp]
    L.lom_profile_match.argtypes = [vp, vp, C.c_size_t, C.c_size_t, fp, fp, C.c_float, C.c_int, dp, dp, dp, dp]
    L.lom_profile_insert.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, dp]
    L.lom_comm_unique_id.argtypes = [C.c_char_p]
    L.lom_comm_init.argtypes = [vp, C.c_int, C.c_int, C.c_char_p]
    L.lom_comm_finalize.argtypes = [vp]
    L.lom_comm_host_id.argtypes = [C.c_char_p]
    L.lom_host_comm_create.argtypes = [C.c_int, C.c_int, C.c_char_p, C.POINTER(vp)]
    L.lom_host_comm_allreduce.argtypes = [vp, dp, C.c_int]
    L.lom_host_comm_destroy.argtypes = [vp]
    L.lom_host_comm_destroy.restype = None
    L.lom_comm_attach_host.argtypes = [vp, vp]
    L.lom_comm_attach_p2p.argtypes = [vp, vp]
    L.lom_comm_attach_p2p.restype = C.c_int
    L.lom_host_comm_allgather.argtypes = [vp, vp, C.c_size_t, vp]
    L.lom_host_comm_allgather.restype = C.c_int
    L.lom_align_with_hooks.argtypes = [C.POINTER(AlignHooks), fp, fp, fp, fp, C.POINTER(AlignStats)]
    L.lom_point_time_normalize.argtypes = [vp, C.c_size_t, vp]
    L.lom_point_time_normalize.restype = None
    L.lom_transform_non_rigid.argtypes = [vp, C.c_size_t, pp, pp, vp]
    L.lom_transform_non_rigid.restype = None
    L.lom_range_filter.argtypes = [vp, vp, C.c_size_t, C.c_float, C.c_float, vp, vp]
    L.lom_range_filter.restype = C.c_size_t
    L.lom_cloud_classify.argtypes = [vp, C.c_size_t, vp, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.lom_cloud_classify.restype = C.c_size_t
    L.lom_odometry_default_params.argtypes = [C.POINTER(OdometryParams)]
    L.lom_odometry_default_params.restype = None
    L.lom_odometry_create.argtypes = [C.POINTER(OdometryParams), C.c_int, C.POINTER(vp)]
    L.lom_odometry_destroy.argtypes = [vp]
    L.lom_odometry_destroy.restype = None
    L.lom_odometry_process_cloud.argtypes = [vp, vp, C.c_size_t]
    L.lom_odometry_hint_next.argtypes = [vp, vp, C.c_size_t]
    L.lom_odometry_process_sequence.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(C.c_size_t)]
    L.lom_odometry_process_batch.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_int)]
    L.lom_odometry_get_pose.argtypes = [vp, pp]
    L.lom_odometry_get_stats.argtypes = [vp, C.POINTER(OdometryFrameStats)]
    L.lom_odometry_get_temp_cloud.argtypes = [vp, vp, C.c_size_t]
    L.lom_odometry_get_temp_cloud.restype = C.c_int64
    L.lom_odometry_debug_set_state.argtypes = [vp, pp, pp]
    L.lom_odometry_keyframe.argtypes = [vp]
    L.lom_odometry_keyframe.restype = vp
    L.lom_odometry_last_error.argtypes = [vp]
    L.lom_odometry_last_error.restype = C.c_char_p
    L.lom_frontend_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    L.lom_frontend_destroy.argtypes = [vp]
    L.lom_frontend_destroy.restype = None
    L.lom_frontend_last_error.argtypes = [vp]
    L.lom_frontend_last_error.restype = C.c_char_p
    L.lom_frontend_process.argtypes = [vp, vp, C.c_size_t, pp, pp, C.c_float, C.c_float]
    L.lom_frontend_results.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint32)]
    L.lom_frontend_wait.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.lom_frontend_fetch.argtypes = [vp, C.c_int, vp, vp, C.c_size_t]
    L.lom_frontend_fetch.restype = C.c_int64
    L.lom_frontend_stream.argtypes = [vp]
    L.lom_frontend_stream.restype = vp
    L.lom_debug_sinf.argtypes = [vp, vp, C.c_size_t, vp]
    L.lom_voxel_downsample_device_nowait.argtypes = [vp, C.c_float, vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(vp),
                                                     C.POINTER(vp), C.POINTER(vp)]
    L.lom_map_read_device_words.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(C.c_uint32)]
    L.lom_map_read_device_words_begin.argtypes = [vp, C.POINTER(vp), C.c_int]
    L.lom_map_read_device_words_end.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.lom_estimate_normals.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_float, C.c_int, vp, vp]
    L.lom_estimate_normals.restype = C.c_int64
    L.lom_pcd_read.argtypes = [C.c_char_p, vp, vp, C.c_size_t, C.POINTER(PcdInfo)]
    L.lom_pcd_read.restype = C.c_int64
    L.lom_pcd_last_error.restype = C.c_char_p
    L.lom_pointcloud2_unpack.argtypes = [C.POINTER(Pc2View), vp, C.c_size_t, C.POINTER(C.c_uint32)]
    L.lom_pointcloud2_unpack.restype = C.c_int64
    L.lom_pointcloud2_layout.argtypes = [C.c_int, C.POINTER(Pc2Field), C.POINTER(C.c_uint32)]
    L.lom_pointcloud2_pack_xyz.argtypes = [vp, C.c_size_t, C.c_size_t, vp, C.c_size_t]
    L.lom_pointcloud2_pack_xyz.restype = C.c_int64
    L.lom_pointcloud2_last_error.restype = C.c_char_p
    L.lom_map_set_option.argtypes = [vp, C.c_int, C.c_int64]
    L.lom_map_debug_counter.argtypes = [vp, C.c_int]
    L.lom_map_debug_counter.restype = C.c_int64
    L.lom_odometry_set_option.argtypes = [vp, C.c_int, C.c_int64]
    L.lom_odometry_debug_counter.argtypes = [vp, C.c_int]
    L.lom_odometry_debug_counter.restype = C.c_int64
    L.lom_frontend_set_option.argtypes = [vp, C.c_int, C.c_int64]
    L.lom_classify_neighbourhood.argtypes = [vp, vp, C.c_size_t, C.POINTER(NeighbourhoodParams), vp, vp, vp]
    L.lom_classify_neighbourhood.restype = C.c_int64
    L.lom_frontend_set_classifier.argtypes = [vp, C.c_int, C.POINTER(NeighbourhoodParams)]
    L.lom_frontend_debug_counter.argtypes = [vp, C.c_int]
    L.lom_frontend_debug_counter.restype = C.c_int64
    L.lom_odometry_set_classifier.argtypes = [vp, C.c_int, C.POINTER(NeighbourhoodParams)]
    for fn in (L.lom_map_carve_rays, L.lom_map_carve_rays_device):
        fn.argtypes = [vp, fp, vp, C.c_size_t, C.c_size_t, C.POINTER(CarveParams), C.POINTER(CarveStats)]
    L.lom_map_carve_counts.argtypes = [vp, fp, vp, C.c_size_t, C.c_size_t, C.POINTER(CarveParams), vp, vp, C.c_size_t]
    L.lom_map_carve_counts.restype = C.c_int64
    L.lom_odometry_set_carve.argtypes = [vp, C.POINTER(CarveParams)]
    L.lom_odometry_get_carve_stats.argtypes = [vp, C.POINTER(CarveStats)]
    L.lom_host_comm_set_timeout.argtypes = [vp, C.c_double]
    L.lom_host_comm_abort.argtypes = [vp]
    L.lom_host_comm_last_error.argtypes = [vp]
    L.lom_host_comm_last_error.restype = C.c_char_p
    L.lom_scan_create.argtypes = [vp, C.POINTER(vp)]
    L.lom_scan_create_on_partition.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.lom_scan_create_on_partition.restype = C.c_int
    L.lom_scan_destroy.argtypes = [vp]
    L.lom_scan_destroy.restype = None
    L.lom_scan_last_error.argtypes = [vp]
    L.lom_scan_last_error.restype = C.c_char_p
    L.lom_scan_set_option.argtypes = [vp, C.c_int, C.c_int64]
    L.lom_scan_set_stream.argtypes = [vp, vp]
    L.lom_scan_get_stream.argtypes = [vp]
    L.lom_scan_get_stream.restype = vp
    L.lom_scan_align.argtypes = L.lom_match_align.argtypes
    L.lom_scan_align_device.argtypes = L.lom_match_align.argtypes
    L.lom_scan_align_repeat.argtypes = L.lom_match_align_repeat.argtypes
    L.lom_scan_find_pairs.argtypes = L.lom_match_find_pairs.argtypes
    L.lom_scan_find_pairs.restype = C.c_int64
    L.lom_scan_find_pairs_sq.argtypes = L.lom_match_find_pairs_sq.argtypes
    L.lom_scan_find_pairs_sq.restype = C.c_int64
    L.lom_quality_from_sums.argtypes = [dp, C.c_int64, C.c_float, C.c_float, C.POINTER(QualityReport)]
    L.lom_match_quality.argtypes = [vp, vp, C.c_size_t, C.c_size_t, fp, fp, C.c_float, C.c_float, C.c_float,
                                    C.POINTER(QualityReport), vp]
    L.lom_match_quality_device.argtypes = L.lom_match_quality.argtypes
    L.lom_scan_quality.argtypes = L.lom_match_quality.argtypes
    L.lom_scan_quality_device.argtypes = L.lom_match_quality.argtypes
    L.lom_match_quality_batch_sums.argtypes = [vp, C.POINTER(QualityProblem), C.c_int, C.c_float, dp]
    L.lom_match_quality_batch_sums_device.argtypes = L.lom_match_quality_batch_sums.argtypes
    L.lom_scan_quality_batch_sums.argtypes = L.lom_match_quality_batch_sums.argtypes
    L.lom_scan_quality_batch_sums_device.argtypes = L.lom_match_quality_batch_sums.argtypes
    L.lom_match_quality_batch.argtypes = [vp, C.POINTER(QualityProblem), C.c_int, C.c_float, C.c_float, C.c_float,
                                          C.POINTER(QualityReport), C.POINTER(C.c_int)]
    L.lom_match_quality_batch_device.argtypes = L.lom_match_quality_batch.argtypes
    L.lom_scan_quality_batch.argtypes = L.lom_match_quality_batch.argtypes
    L.lom_scan_quality_batch_device.argtypes = L.lom_match_quality_batch.argtypes
    L.lom_quality_batch_best.argtypes = [C.POINTER(QualityReport), C.c_int]
    L.lom_pose_lattice.argtypes = [pp, fp, fp, C.c_float, C.c_float, pp, C.c_int]
    L.lom_odometry_set_quality_thresholds.argtypes = [vp, C.c_float, C.c_float]
    L.lom_odometry_get_quality.argtypes = [vp, C.POINTER(QualityReport)]
    plp = C.POINTER(PlaceParams)
    L.lom_place_db_create.argtypes = [plp, C.c_int, C.c_size_t, C.POINTER(vp)]
    L.lom_place_db_destroy.argtypes = [vp]
    L.lom_place_db_destroy.restype = None
    L.lom_place_db_last_error.argtypes = [vp]
    L.lom_place_db_last_error.restype = C.c_char_p
    L.lom_place_db_size.argtypes = [vp]
    L.lom_place_db_size.restype = C.c_int64
    L.lom_place_db_clear.argtypes = [vp]
    L.lom_place_db_params.argtypes = [vp, plp]
    L.lom_place_db_stream.argtypes = [vp]
    L.lom_place_db_stream.restype = vp
    L.lom_place_db_device.argtypes = [vp]
    L.lom_place_db_wait_event.argtypes = [vp, vp]
    L.lom_place_describe.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
    L.lom_place_describe_device.argtypes = L.lom_place_describe.argtypes
    L.lom_place_db_add.argtypes = [vp, vp]
    L.lom_place_db_add.restype = C.c_int64
    L.lom_place_db_add_cloud.argtypes = [vp, vp, C.c_size_t, C.c_size_t]
    L.lom_place_db_add_cloud.restype = C.c_int64
    L.lom_place_db_add_cloud_device.argtypes = L.lom_place_db_add_cloud.argtypes
    L.lom_place_db_add_cloud_device.restype = C.c_int64
    L.lom_place_db_get.argtypes = [vp, C.c_int64, vp]
    L.lom_place_db_query.argtypes = [vp, vp, C.c_int, C.c_int64, C.c_int64, C.c_int, vp, vp]
    L.lom_place_db_query_cloud_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int64, C.c_int64, C.c_int, vp]
    L.lom_place_shift_yaw.argtypes = [plp, C.c_uint32]
    L.lom_place_shift_yaw.restype = C.c_double
    L.lom_odometry_place_descriptor.argtypes = [vp, vp, C.c_int, vp, C.POINTER(C.c_int64)]
    L.lom_frontend_deskewed.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint32)]
    L.lom_graph_create.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.lom_graph_destroy.argtypes = [vp]
    L.lom_graph_destroy.restype = None
    L.lom_graph_last_error.argtypes = [vp]
    L.lom_graph_last_error.restype = C.c_char_p
    L.lom_graph_clear.argtypes = [vp]
    L.lom_graph_stream.argtypes = [vp]
    L.lom_graph_stream.restype = vp
    L.lom_graph_device.argtypes = [vp]
    L.lom_graph_add_node.argtypes = [vp, vp, C.c_int]
    L.lom_graph_add_nodes.argtypes = [vp, vp, vp, C.c_size_t]
    L.lom_graph_add_edge.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, C.c_double]
    L.lom_graph_add_edges.argtypes = [vp, vp, vp, vp, vp, C.c_size_t]
    for fn in (L.lom_graph_add_node, L.lom_graph_add_nodes, L.lom_graph_add_edge, L.lom_graph_add_edges):
        fn.restype = C.c_int64
    L.lom_graph_node_count.argtypes = [vp]
    L.lom_graph_node_count.restype = C.c_int64
    L.lom_graph_edge_count.argtypes = [vp]
    L.lom_graph_edge_count.restype = C.c_int64
    L.lom_graph_get_poses.argtypes = [vp, C.c_int64, C.c_int64, vp]
    L.lom_graph_set_pose.argtypes = [vp, C.c_int64, vp]
    L.lom_graph_set_fixed.argtypes = [vp, C.c_int64, C.c_int]
    L.lom_graph_optimize.argtypes = [vp, C.POINTER(GraphParams), C.POINTER(GraphStats)]
    L.lom_graph_evaluate.argtypes = [vp, C.c_double, vp, vp, vp, vp, vp]
    L.lom_graph_debug_matvec.argtypes = [vp, C.c_double, vp, vp]
    L.lom_graph_edge_chi2.argtypes = [vp, C.c_int64, C.c_int64, vp]
    L.lom_graph_check_gauge.argtypes = [C.c_int64, vp, C.c_int64, vp, C.POINTER(C.c_int64)]
    L.lom_graph_lm_policy.argtypes = [C.c_double, C.c_double, C.c_double, dp, dp, dp]
    L.lom_graph_information_from_quality.argtypes = [C.POINTER(QualityReport), C.c_int, vp]
    L.lom_graph_pose_from_f32.argtypes = [pp, vp]
    L.lom_graph_pose_to_f32.argtypes = [vp, pp]
    L.lom_archive_create.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.lom_archive_destroy.argtypes = [vp]
    L.lom_archive_destroy.restype = None
    L.lom_archive_last_error.argtypes = [vp]
    L.lom_archive_last_error.restype = C.c_char_p
    L.lom_archive_clear.argtypes = [vp]
    L.lom_archive_stream.argtypes = [vp]
    L.lom_archive_stream.restype = vp
    L.lom_archive_device.argtypes = [vp]
    L.lom_archive_wait_event.argtypes = [vp, vp]
    L.lom_archive_add.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t]
    L.lom_archive_add_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp]
    L.lom_archive_scan_count.argtypes = [vp]
    L.lom_archive_point_count.argtypes = [vp]
    L.lom_archive_scan_size.argtypes = [vp, C.c_int64]
    L.lom_archive_get.argtypes = [vp, C.c_int64, vp, vp, C.c_size_t]
    for fn in (L.lom_archive_add, L.lom_archive_add_device, L.lom_archive_scan_count, L.lom_archive_point_count,
               L.lom_archive_scan_size, L.lom_archive_get):
        fn.restype = C.c_int64
    L.lom_map_assemble.argtypes = [vp, vp, vp, vp, C.c_size_t, C.POINTER(AssembleParams), C.POINTER(AssembleStats)]
    L.lom_graph_pose_rotation_matrix.argtypes = [vp, vp]
    L.lom_odometry_archive_scan.argtypes = [vp, vp, C.POINTER(C.c_int64)]
    L.lom_odometry_rebuild_keyframe.argtypes = [vp, vp, vp, vp, C.c_size_t, pp, C.POINTER(AssembleStats)]
    L.lom_map_carve_scans.argtypes = [vp, vp, vp, vp, C.c_size_t, C.POINTER(VoteParams), C.POINTER(VoteStats)]
    L.lom_map_scan_votes.argtypes = [vp, vp, vp, vp, C.c_size_t, C.POINTER(VoteParams), vp, vp, C.c_size_t]
    L.lom_map_scan_votes.restype = C.c_int64
    L.lom_odometry_set_rebuild_votes.argtypes = [vp, C.POINTER(VoteParams)]
    L.lom_odometry_get_rebuild_vote_stats.argtypes = [vp, C.POINTER(VoteStats)]
    L.lom_archive_add_points.argtypes = [vp, vp, C.c_size_t, C.c_size_t]
    L.lom_archive_add_points_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
    L.lom_archive_add_points.restype = L.lom_archive_add_points_device.restype = C.c_int64
    L.lom_odometry_archive_deskewed.argtypes = [vp, vp, C.POINTER(C.c_int64)]
    L.lom_odometry_occupancy_scan.argtypes = [vp, vp, C.POINTER(OccupancyRayParams), C.POINTER(OccupancyStats)]
    L.lom_occupancy_create.argtypes = [C.POINTER(OccupancyGeometry), C.c_int, C.POINTER(vp)]
    L.lom_occupancy_destroy.argtypes = [vp]
    L.lom_occupancy_destroy.restype = None
    L.lom_occupancy_last_error.argtypes = [vp]
    L.lom_occupancy_last_error.restype = C.c_char_p
    L.lom_occupancy_clear.argtypes = [vp]
    L.lom_occupancy_get_geometry.argtypes = [vp, C.POINTER(OccupancyGeometry)]
    L.lom_occupancy_stream.argtypes = [vp]
    L.lom_occupancy_stream.restype = vp
    L.lom_occupancy_device.argtypes = [vp]
    L.lom_occupancy_wait_event.argtypes = [vp, vp]
    L.lom_occupancy_set_option.argtypes = [vp, C.c_int, C.c_int64]
    L.lom_occupancy_integrate.argtypes = [vp, vp, vp, vp, C.c_size_t, C.POINTER(OccupancyRayParams), C.POINTER(OccupancyStats)]
    L.lom_occupancy_integrate_cloud.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.POINTER(OccupancyRayParams),
                                                C.POINTER(OccupancyStats)]
    L.lom_occupancy_integrate_cloud_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.POINTER(OccupancyRayParams), vp,
                                                       C.POINTER(OccupancyStats)]
    L.lom_occupancy_counts.argtypes = [vp, vp, vp, C.c_size_t]
    L.lom_occupancy_counts.restype = C.c_int64
    L.lom_occupancy_classify.argtypes = [vp, C.POINTER(OccupancyRule), vp, C.c_size_t, C.POINTER(OccupancySummary)]
    L.lom_occupancy_classify_device.argtypes = [vp, C.POINTER(OccupancyRule), C.POINTER(vp)]
    L.lom_odometry_elevation_scan.argtypes = [vp, vp, C.POINTER(ElevationPointParams), C.POINTER(ElevationStats)]
    L.lom_elevation_create.argtypes = [C.POINTER(ElevationGeometry), C.c_int, C.POINTER(vp)]
    L.lom_elevation_destroy.argtypes = [vp]
    L.lom_elevation_destroy.restype = None
    L.lom_elevation_last_error.argtypes = [vp]
    L.lom_elevation_last_error.restype = C.c_char_p
    L.lom_elevation_clear.argtypes = [vp]
    L.lom_elevation_get_geometry.argtypes = [vp, C.POINTER(ElevationGeometry)]
    L.lom_elevation_stream.argtypes = [vp]
    L.lom_elevation_stream.restype = vp
    L.lom_elevation_device.argtypes = [vp]
    L.lom_elevation_wait_event.argtypes = [vp, vp]
    L.lom_elevation_set_option.argtypes = [vp, C.c_int, C.c_int64]
    L.lom_elevation_integrate.argtypes = [vp, vp, vp, vp, C.c_size_t, C.POINTER(ElevationPointParams), C.POINTER(ElevationStats)]
    L.lom_elevation_integrate_cloud.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.POINTER(ElevationPointParams),
                                                C.POINTER(ElevationStats)]
    L.lom_elevation_integrate_cloud_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.POINTER(ElevationPointParams), vp,
                                                       C.POINTER(ElevationStats)]
    L.lom_elevation_cells.argtypes = [vp, vp, vp, vp, vp, C.c_size_t]
    L.lom_elevation_cells.restype = C.c_int64
    L.lom_elevation_layers.argtypes = [vp, C.POINTER(ElevationLayerParams), vp, vp, vp, vp, vp, vp, C.c_size_t]
    L.lom_elevation_cost.argtypes = [vp, C.POINTER(ElevationLayerParams), C.POINTER(ElevationCostParams), vp, C.c_size_t,
                                     C.POINTER(ElevationSummary)]
    L.lom_elevation_cost_device.argtypes = [vp, C.POINTER(ElevationLayerParams), C.POINTER(ElevationCostParams), C.POINTER(vp)]
    L.lom_clearance_create.argtypes = [C.POINTER(OccupancyGeometry), C.c_int, C.POINTER(vp)]
    L.lom_clearance_destroy.argtypes = [vp]
    L.lom_clearance_destroy.restype = None
    L.lom_clearance_last_error.argtypes = [vp]
    L.lom_clearance_last_error.restype = C.c_char_p
    L.lom_clearance_clear.argtypes = [vp]
    L.lom_clearance_get_geometry.argtypes = [vp, C.POINTER(OccupancyGeometry)]
    L.lom_clearance_stream.argtypes = [vp]
    L.lom_clearance_stream.restype = vp
    L.lom_clearance_device.argtypes = [vp]
    L.lom_clearance_wait_event.argtypes = [vp, vp]
    L.lom_clearance_set_option.argtypes = [vp, C.c_int, C.c_int64]
    L.lom_clearance_update.argtypes = [vp, vp, vp, C.POINTER(ClearanceParams), C.POINTER(ClearanceWindow), C.POINTER(ClearanceSummary)]
    L.lom_clearance_update_device.argtypes = [vp, vp, vp, vp, C.POINTER(ClearanceParams), C.POINTER(ClearanceWindow),
                                              C.POINTER(ClearanceSummary)]
    L.lom_clearance_update_from_grids.argtypes = [vp, vp, C.POINTER(OccupancyRule), vp, C.POINTER(ElevationLayerParams),
                                                  C.POINTER(ElevationCostParams), C.POINTER(ClearanceParams),
                                                  C.POINTER(ClearanceWindow), C.POINTER(ClearanceSummary)]
    L.lom_clearance_cost.argtypes = [vp, vp, C.c_size_t, C.POINTER(ClearanceSummary)]
    L.lom_clearance_cost_device.argtypes = [vp, C.POINTER(vp)]
    L.lom_clearance_distance_sq.argtypes = [vp, vp, C.c_size_t]
    L.lom_clearance_distance.argtypes = [vp, vp, C.c_size_t]
    L.lom_clearance_cost_table.argtypes = [C.POINTER(ClearanceParams), C.POINTER(OccupancyGeometry), vp, C.c_size_t]
    L.lom_clearance_cost_table.restype = C.c_int64
    L.lom_clearance_query.argtypes = [vp, vp, C.c_size_t, vp, vp]
    L.lom_navfield_create.argtypes = [C.POINTER(OccupancyGeometry), C.c_int, C.POINTER(vp)]
    L.lom_navfield_destroy.argtypes = [vp]
    L.lom_navfield_destroy.restype = None
    L.lom_navfield_last_error.argtypes = [vp]
    L.lom_navfield_last_error.restype = C.c_char_p
    L.lom_navfield_clear.argtypes = [vp]
    L.lom_navfield_get_geometry.argtypes = [vp, C.POINTER(OccupancyGeometry)]
    L.lom_navfield_stream.argtypes = [vp]
    L.lom_navfield_stream.restype = vp
    L.lom_navfield_device.argtypes = [vp]
    L.lom_navfield_wait_event.argtypes = [vp, vp]
    L.lom_navfield_set_option.argtypes = [vp, C.c_int, C.c_int64]
    L.lom_navfield_solve.argtypes = [vp, vp, C.POINTER(NavFieldParams), C.c_int, vp, C.c_size_t, C.POINTER(NavFieldSummary)]
    L.lom_navfield_solve_device.argtypes = [vp, vp, vp, C.POINTER(NavFieldParams), C.c_int, vp, C.c_size_t, C.POINTER(NavFieldSummary)]
    L.lom_navfield_solve_from_clearance.argtypes = [vp, vp, C.POINTER(NavFieldParams), C.c_int, vp, C.c_size_t,
                                                    C.POINTER(NavFieldSummary)]
    L.lom_navfield_potential.argtypes = [vp, vp, C.c_size_t]
    L.lom_navfield_potential_device.argtypes = [vp, C.POINTER(vp)]
    L.lom_navfield_paths.argtypes = [vp, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp]
    L.lom_navfield_query.argtypes = [vp, vp, C.c_size_t, vp]
    L.lom_navfield_cell_costs.argtypes = [C.POINTER(NavFieldParams), vp]
    L.lom_navfield_stats.argtypes = [vp, C.POINTER(NavFieldSolveStats)]
    L.lom_regions_create.argtypes = [C.POINTER(OccupancyGeometry), C.c_int, C.POINTER(vp)]
    L.lom_regions_destroy.argtypes = [vp]
    L.lom_regions_destroy.restype = None
    L.lom_regions_last_error.argtypes = [vp]
    L.lom_regions_last_error.restype = C.c_char_p
    L.lom_regions_clear.argtypes = [vp]
    L.lom_regions_get_geometry.argtypes = [vp, C.POINTER(OccupancyGeometry)]
    L.lom_regions_stream.argtypes = [vp]
    L.lom_regions_stream.restype = vp
    L.lom_regions_device.argtypes = [vp]
    L.lom_regions_wait_event.argtypes = [vp, vp]
    L.lom_regions_set_option.argtypes = [vp, C.c_int, C.c_int64]
    L.lom_regions_extract.argtypes = [vp, vp, vp, vp, C.POINTER(RegionsParams), C.POINTER(RegionsSummary)]
    L.lom_regions_extract_device.argtypes = [vp, vp, vp, vp, vp, C.POINTER(RegionsParams), C.POINTER(RegionsSummary)]
    L.lom_regions_extract_from_grids.argtypes = [vp, vp, C.POINTER(OccupancyRule), vp, vp, C.POINTER(RegionsParams),
                                                 C.POINTER(RegionsSummary)]
    L.lom_regions_labels.argtypes = [vp, vp, C.c_size_t]
    L.lom_regions_labels_device.argtypes = [vp, C.POINTER(vp)]
    L.lom_regions_list.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lom_regions_goals.argtypes = [vp, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lom_regions_query.argtypes = [vp, vp, C.c_size_t, vp]
    L.lom_regions_stats.argtypes = [vp, C.POINTER(RegionsExtractStats)]
    L.lom_visibility_create.argtypes = [C.POINTER(OccupancyGeometry), C.c_int, C.POINTER(vp)]
    L.lom_visibility_destroy.argtypes = [vp]
    L.lom_visibility_destroy.restype = None
    L.lom_visibility_last_error.argtypes = [vp]
    L.lom_visibility_last_error.restype = C.c_char_p
    L.lom_visibility_clear.argtypes = [vp]
    L.lom_visibility_get_geometry.argtypes = [vp, C.POINTER(OccupancyGeometry)]
    L.lom_visibility_stream.argtypes = [vp]
    L.lom_visibility_stream.restype = vp
    L.lom_visibility_device.argtypes = [vp]
    L.lom_visibility_wait_event.argtypes = [vp, vp]
    L.lom_visibility_set_option.argtypes = [vp, C.c_int, C.c_int64]
    L.lom_visibility_table.argtypes = [C.c_uint32, vp]
    L.lom_visibility_cast.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(VisibilityParams), C.POINTER(VisibilitySummary)]
    L.lom_visibility_cast_device.argtypes = [vp, vp, vp, vp, C.c_size_t, C.POINTER(VisibilityParams), C.POINTER(VisibilitySummary)]
    L.lom_visibility_cast_from_occupancy.argtypes = [vp, vp, C.POINTER(OccupancyRule), vp, C.c_size_t, C.POINTER(VisibilityParams),
                                                     C.POINTER(VisibilitySummary)]
    L.lom_visibility_records.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lom_visibility_beams.argtypes = [vp, vp, C.c_size_t]
    L.lom_visibility_windows_device.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.lom_visibility_windows.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lom_visibility_select.argtypes = [vp, C.POINTER(VisibilitySelectParams), vp, vp, C.POINTER(C.c_size_t)]
    L.lom_visibility_select_from_navfield.argtypes = [vp, vp, C.POINTER(VisibilitySelectParams), vp, C.POINTER(C.c_size_t)]
    L.lom_visibility_stats.argtypes = [vp, C.POINTER(VisibilityCallStats)]
    L.lom_rollout_create.argtypes = [C.POINTER(OccupancyGeometry), C.c_int, C.POINTER(vp)]
    L.lom_rollout_destroy.argtypes = [vp]
    L.lom_rollout_destroy.restype = None
    L.lom_rollout_last_error.argtypes = [vp]
    L.lom_rollout_last_error.restype = C.c_char_p
    L.lom_rollout_clear.argtypes = [vp]
    L.lom_rollout_get_geometry.argtypes = [vp, C.POINTER(OccupancyGeometry)]
    L.lom_rollout_stream.argtypes = [vp]
    L.lom_rollout_stream.restype = vp
    L.lom_rollout_device.argtypes = [vp]
    L.lom_rollout_wait_event.argtypes = [vp, vp]
    L.lom_rollout_set_option.argtypes = [vp, C.c_int, C.c_int64]
    # states, m, commands, k, footprint, f, params, picks, summary: the tail of every evaluate form
    tail = [vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(RolloutParams), vp, C.POINTER(RolloutSummary)]
    L.lom_rollout_evaluate.argtypes = [vp, vp, vp] + tail
    L.lom_rollout_evaluate_device.argtypes = [vp, vp, vp, vp, vp] + tail
    L.lom_rollout_evaluate_from_grids.argtypes = [vp, vp, vp] + tail
    L.lom_rollout_records.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lom_rollout_stats.argtypes = [vp, C.POINTER(RolloutCallStats)]
    L.lom_rollout_footprint_rectangle.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int, vp, C.c_size_t,
                                                  C.POINTER(C.c_size_t)]
    L.lom_rollout_state_from_pose.argtypes = [C.POINTER(OccupancyGeometry), C.c_float, C.c_float, C.c_float, vp]
    L.lom_rollout_poses.argtypes = [C.POINTER(RolloutParams), vp, vp, vp]
    _lib = L
    return L


def pin_to_device_numa_node(device=0):
    """Restrict this process to the CPUs of the NUMA node the GPU is attached to (no-op when sysfs
    does not tell).  Returns the cpu set used, or None."""
    buf = C.create_string_buffer(512)
    if lib().lom_device_local_cpus(int(device), buf, 512) != 0 or not buf.value:
        return None
    cpus = set()
    for part in buf.value.decode().split(","):
        lo, _, hi = part.partition("-")
        cpus.update(range(int(lo), int(hi or lo) + 1))
    cpus &= os.sched_getaffinity(0)
    if not cpus:
        return None
    os.sched_setaffinity(0, cpus)
    return cpus


def f3(a):
    return (C.c_float * 3)(*[float(v) for v in a])


def f4(a):
    return (C.c_float * 4)(*[float(v) for v in a])


def xyz_array(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("expected an (n, 3) float32 array")
    return a


def replayed_iterations(handle):
    """lom_debug_replayed_iterations: outer iterations of the last device-resident align on `handle` (a map or a scan
    context) that the replay fold accounted for without running them."""
    return int(check(lib().lom_debug_replayed_iterations(handle), handle))


def set_host_replay_fold(on):
    """lom_debug_set_host_replay_fold: the host driver's replay fold, process-wide; returns the previous setting."""
    return int(lib().lom_debug_set_host_replay_fold(int(bool(on))))


def check(rc, handle=None):
    if rc < 0:
        text = lib().lom_last_error(handle)
        raise LomError(int(rc), text.decode() if text else "")
    return rc
