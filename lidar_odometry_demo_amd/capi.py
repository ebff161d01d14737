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


class NavFieldResolveCounters(C.Structure):
    """lom_navfield_resolve_counters"""
    _fields_ = [("cells_changed", C.c_uint64), ("cells_raised", C.c_uint64), ("raise_launches", C.c_uint64),
                ("relax_launches", C.c_uint64), ("waits", C.c_uint64), ("tiles_marked", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class NavFieldShiftCounters(C.Structure):
    """lom_navfield_shift_counters"""
    _fields_ = [("cells_kept", C.c_uint64), ("cells_entered", C.c_uint64), ("goals_left", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class NavFieldWaypointParams(C.Structure):
    """lom_navfield_waypoint_params"""
    _fields_ = [("max_cell_cost", C.c_uint32), ("lookahead", C.c_uint32), ("route_cap", C.c_uint32), ("flags", C.c_uint32)]


assert C.sizeof(NavFieldParams) == 20 and C.sizeof(NavFieldSummary) == 64 and C.sizeof(NavFieldSolveStats) == 24
assert C.sizeof(NavFieldResolveCounters) == 48 and C.sizeof(NavFieldWaypointParams) == 16
assert C.sizeof(NavFieldShiftCounters) == 24
NAV_UNREACHED, NAV_MAX = 0xFFFFFFFF, 0xFFFFFFFE
NAV_UNKNOWN_PASSABLE = 1
NAV_CELLS, NAV_METRES = 0, 1
NAV_OPT_TEST_INNER_CAP, NAV_OPT_TEST_BATCH, NAV_OPT_TEST_ALL_TILES, NAV_OPT_TEST_RESOLVE_FORM = 1, 2, 3, 4
NAV_OPT_TEST_SHORTCUT_SERIAL = 5


class NavSetSolveStats(C.Structure):
    """lom_navset_solve_stats"""
    _fields_ = [("launches", C.c_uint64), ("waits", C.c_uint64), ("tiles", C.c_uint64), ("fields", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(NavSetSolveStats) == 32
NAVSET_NO_OWNER, NAVSET_MAX_FIELDS = 0xFFFF, 65535
NAVSET_OPT_TEST_INNER_CAP, NAVSET_OPT_TEST_BATCH, NAVSET_OPT_TEST_ALL_TILES = 1, 2, 3


class PoseFieldParams(C.Structure):
    """lom_posefield_params"""
    _fields_ = [("nav", NavFieldParams), ("turn_cost", C.c_uint32), ("spin_cost", C.c_uint32), ("reverse_cost", C.c_uint32),
                ("flags", C.c_uint32)]


class PoseFieldSummary(C.Structure):
    """lom_posefield_summary"""
    _fields_ = [("states_blocked", C.c_uint64), ("states_reached", C.c_uint64), ("states_unreached", C.c_uint64),
                ("cells_reached", C.c_uint64), ("cells_invalid", C.c_uint64), ("goals_used", C.c_uint64),
                ("goals_rejected", C.c_uint64), ("range_exceeded", C.c_uint64), ("max_potential", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class PoseFieldSolveStats(C.Structure):
    """lom_posefield_solve_stats"""
    _fields_ = [("launches", C.c_uint64), ("waits", C.c_uint64), ("tiles", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class PoseFieldResolveCounters(C.Structure):
    """lom_posefield_resolve_counters"""
    _fields_ = [("cells_changed", C.c_uint64), ("states_changed", C.c_uint64), ("states_raised", C.c_uint64),
                ("raise_launches", C.c_uint64), ("relax_launches", C.c_uint64), ("waits", C.c_uint64), ("tiles_marked", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(PoseFieldParams) == 36 and C.sizeof(PoseFieldSummary) == 72 and C.sizeof(PoseFieldSolveStats) == 24
assert C.sizeof(PoseFieldResolveCounters) == 56
POSE_HEADINGS = 8
POSE_SPIN, POSE_REVERSE = 1, 2
POSE_OPT_TEST_INNER_CAP, POSE_OPT_TEST_BATCH, POSE_OPT_TEST_ALL_TILES, POSE_OPT_TEST_RESOLVE_FORM = 1, 2, 3, 4


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


# ---- the prototypes: every function include/lidar_odometry_amd.h declares, name -> (restype, argtypes).  lib() applies the
# table as it is; tests/test_capi_prototypes.py holds it against the header (return type and parameter count).
_P = C.POINTER
_int, _i64, _size, _u32, _float, _double, _str = C.c_int, C.c_int64, C.c_size_t, C.c_uint32, C.c_float, C.c_double, C.c_char_p
_fp, _dp, _pp, _vp = _P(C.c_float), _P(C.c_double), _P(Pose), C.c_void_p
IDLE_HOOK_FN = C.CFUNCTYPE(None, C.c_void_p)  # lom_map_set_align_idle_hook


def _family(stem, create_args):
    """create / destroy / last_error of the handle family lom_<stem>_*; create_args: what comes before the handle out"""
    return {f"lom_{stem}_create": (_int, [*create_args, _P(_vp)]), f"lom_{stem}_destroy": (None, [_vp]),
            f"lom_{stem}_last_error": (_str, [_vp])}


def _grid_family(stem, geometry):
    """the ten entry points every grid family has"""
    return {**_family(stem, [_P(geometry), _int]), f"lom_{stem}_clear": (_int, [_vp]),
            f"lom_{stem}_shift": (_int, [_vp, C.c_int32, C.c_int32]),
            f"lom_{stem}_get_geometry": (_int, [_vp, _P(geometry)]), f"lom_{stem}_stream": (_vp, [_vp]),
            f"lom_{stem}_device": (_int, [_vp]), f"lom_{stem}_wait_event": (_int, [_vp, _vp]),
            f"lom_{stem}_set_option": (_int, [_vp, _int, _i64])}


# argument lists that several entry points share: a map's and a scan context's forms, host and device
_ADD = [_vp, _vp, _vp, _size, _size]
_PAIRS = [_vp, _vp, _size, _size, _fp, _fp, _float, _vp]
_PAIRS_SQ = [_vp, _vp, _size, _size, _fp, _fp, _double, _vp]
_ALIGN = [_vp, _vp, _size, _size, _fp, _fp, _fp, _fp, _P(AlignStats)]
_ALIGN_REPEAT = [_vp, _vp, _size, _size, _fp, _fp, _int, _fp, _fp, _P(AlignStats)]
_ALIGN_BATCH = [_vp, _P(AlignProblem), _int, _P(AlignResult), _P(_int)]
_ALIGN_MULTI = [_vp, _P(AlignMultiProblem), _int, _P(AlignResult), _P(_int)]
_QUALITY = [_vp, _vp, _size, _size, _fp, _fp, _float, _float, _float, _P(QualityReport), _vp]
_QUALITY_BATCH_SUMS = [_vp, _P(QualityProblem), _int, _float, _dp]
_QUALITY_BATCH = [_vp, _P(QualityProblem), _int, _float, _float, _float, _P(QualityReport), _P(_int)]
_CARVE = [_vp, _fp, _vp, _size, _size, _P(CarveParams), _P(CarveStats)]
_DESCRIBE = [_vp, _vp, _size, _size, _vp]
_ADD_CLOUD = [_vp, _vp, _size, _size]
_CLASSIFIER = [_vp, _int, _P(NeighbourhoodParams)]
_OPTION = [_vp, _int, _i64]
# states, m, commands, k, footprint, f, params, picks, summary: the tail of every rollout evaluate form
_ROLLOUT_TAIL = [_vp, _size, _vp, _size, _vp, _size, _P(RolloutParams), _vp, _P(RolloutSummary)]

PROTOTYPES = {
    "lom_abi_version": (_int, []),
    "lom_device_count": (_int, []),
    "lom_device_local_cpus": (_int, [_int, _str, _size]),
    "lom_pose_identity": (None, [_pp]),
    "lom_pose_compose": (None, [_pp, _pp, _pp]),
    "lom_pose_inverse": (None, [_pp, _pp]),
    "lom_pose_relative_to": (None, [_pp, _pp, _pp]),
    "lom_pose_rotation_matrix": (None, [_pp, _fp]),
    "lom_transform_points": (_int, [_pp, _vp, _vp, _size, _size, _vp, _vp, _size]),
    # ---- the map (its last error is lom_last_error) and what runs on it
    "lom_map_create": (_int, [_float, _size, _size, _int, _P(_vp)]),
    "lom_map_destroy": (None, [_vp]),
    "lom_last_error": (_str, [_vp]),
    "lom_map_clear": (_int, [_vp, _float]),
    "lom_map_set_max_points": (_int, [_vp, _size]),
    "lom_map_add_points": (_int, _ADD),
    "lom_map_add_points_device": (_int, _ADD),
    "lom_map_add_points_device_nowait": (_int, _ADD),
    "lom_map_status": (_int, [_vp]),
    "lom_map_status_words": (_int, [_vp, _P(_vp), _P(_vp), _P(_u32)]),
    "lom_map_radius_cleanup": (_int, [_vp, _fp, _float]),
    "lom_map_radius_cleanup_after_align": (_int, [_vp, _float]),
    "lom_map_size": (_i64, [_vp]),
    "lom_map_point_count": (_i64, [_vp]),
    "lom_map_export": (_i64, [_vp, _int, _vp, _vp, _size]),
    "lom_map_carve_rays": (_int, _CARVE),
    "lom_map_carve_rays_device": (_int, _CARVE),
    "lom_map_carve_counts": (_i64, [_vp, _fp, _vp, _size, _size, _P(CarveParams), _vp, _vp, _size]),
    "lom_voxel_downsample": (_i64, [_vp, _float, _vp, _vp, _size, _size, _vp, _vp, _size]),
    "lom_upload_points": (_int, [_vp, _vp, _vp, _size, _size, _P(_vp), _P(_vp)]),
    "lom_voxel_downsample_device": (_i64, [_vp, _float, _vp, _vp, _size, _size, _P(_vp), _P(_vp)]),
    "lom_voxel_downsample_device_nowait": (_int, [_vp, _float, _vp, _vp, _size, _vp, _size, _P(_vp), _P(_vp), _P(_vp)]),
    "lom_map_read_device_words": (_int, [_vp, _P(_vp), _int, _P(_u32)]),
    "lom_map_read_device_words_begin": (_int, [_vp, _P(_vp), _int]),
    "lom_map_read_device_words_end": (_int, [_vp, _P(_u32)]),
    "lom_transform_points_device": (_int, [_vp, _vp, _vp, _vp, _size, _size, _P(_vp), _P(_vp)]),
    "lom_match_find_pairs": (_i64, _PAIRS),
    "lom_match_find_pairs_sq": (_i64, _PAIRS_SQ),
    "lom_debug_find_pairs_after": (_i64, [_vp, _vp, _size, _size, _fp, _fp, _fp, _fp, _float, _vp]),
    "lom_match_align": (_int, _ALIGN),
    "lom_match_align_device": (_int, _ALIGN),
    "lom_match_align_repeat": (_int, _ALIGN_REPEAT),
    "lom_match_align_batch": (_int, _ALIGN_BATCH),
    "lom_match_align_batch_device": (_int, _ALIGN_BATCH),
    "lom_align_batch_best": (_int, [_P(AlignResult), _int]),
    "lom_match_align_multi": (_int, _ALIGN_MULTI),
    "lom_match_align_multi_device": (_int, _ALIGN_MULTI),
    "lom_debug_match_stamps": (_int, [_vp, _vp, _size, _size, _fp, _fp, _float, _vp, _size, _P(_u32)]),
    "lom_debug_eval_sums": (_int, [_vp, _vp, _size, _size, _fp, _fp, _dp, _dp, _dp]),
    "lom_debug_lm_trace": (_int, [_vp, _vp, _size, _size, _fp, _fp, _int, _dp, _P(_int), _fp, _fp, _P(AlignStats)]),
    "lom_debug_replayed_iterations": (_int, [_vp]),
    "lom_debug_set_host_replay_fold": (_int, [_int]),
    "lom_debug_replay_fold_count": (_int, [_int, _double]),
    "lom_debug_lm_policy": (_int, [_int, _int, _P(_int), _dp, _dp, _dp, _P(_int), _dp, _P(_int), _P(_int), _dp, _dp]),
    "lom_map_set_profiling": (_int, [_vp, _int]),
    "lom_profile_match": (_int, [_vp, _vp, _size, _size, _fp, _fp, _float, _int, _dp, _dp, _dp, _dp]),
    "lom_profile_insert": (_int, [_vp, _vp, _vp, _size, _size, _dp]),
    "lom_map_set_option": (_int, _OPTION),
    "lom_map_debug_counter": (_i64, [_vp, _int]),
    "lom_map_wait_event": (_int, [_vp, _vp]),
    "lom_map_set_align_idle_hook": (_int, [_vp, IDLE_HOOK_FN, _vp]),
    "lom_map_set_stream": (_int, [_vp, _vp]),
    "lom_map_get_stream": (_vp, [_vp]),
    # ---- scan contexts
    **_family("scan", [_vp]),
    "lom_scan_create_on_partition": (_int, [_vp, _int, _int, _P(_vp)]),
    "lom_scan_set_option": (_int, _OPTION),
    "lom_scan_set_stream": (_int, [_vp, _vp]),
    "lom_scan_get_stream": (_vp, [_vp]),
    "lom_scan_align": (_int, _ALIGN),
    "lom_scan_align_device": (_int, _ALIGN),
    "lom_scan_align_repeat": (_int, _ALIGN_REPEAT),
    "lom_scan_align_batch": (_int, _ALIGN_BATCH),
    "lom_scan_align_batch_device": (_int, _ALIGN_BATCH),
    "lom_scan_find_pairs": (_i64, _PAIRS),
    "lom_scan_find_pairs_sq": (_i64, _PAIRS_SQ),
    # ---- quality reports
    "lom_quality_from_sums": (_int, [_dp, _i64, _float, _float, _P(QualityReport)]),
    "lom_match_quality": (_int, _QUALITY),
    "lom_match_quality_device": (_int, _QUALITY),
    "lom_scan_quality": (_int, _QUALITY),
    "lom_scan_quality_device": (_int, _QUALITY),
    "lom_match_quality_batch_sums": (_int, _QUALITY_BATCH_SUMS),
    "lom_match_quality_batch_sums_device": (_int, _QUALITY_BATCH_SUMS),
    "lom_scan_quality_batch_sums": (_int, _QUALITY_BATCH_SUMS),
    "lom_scan_quality_batch_sums_device": (_int, _QUALITY_BATCH_SUMS),
    "lom_match_quality_batch": (_int, _QUALITY_BATCH),
    "lom_match_quality_batch_device": (_int, _QUALITY_BATCH),
    "lom_scan_quality_batch": (_int, _QUALITY_BATCH),
    "lom_scan_quality_batch_device": (_int, _QUALITY_BATCH),
    "lom_quality_batch_best": (_int, [_P(QualityReport), _int]),
    "lom_pose_lattice": (_int, [_pp, _fp, _fp, _float, _float, _pp, _int]),
    # ---- communicators and hooks
    "lom_comm_unique_id": (_int, [_str]),
    "lom_comm_init": (_int, [_vp, _int, _int, _str]),
    "lom_comm_finalize": (_int, [_vp]),
    "lom_comm_host_id": (_int, [_str]),
    **_family("host_comm", [_int, _int, _str]),
    "lom_host_comm_allreduce": (_int, [_vp, _dp, _int]),
    "lom_host_comm_set_timeout": (_int, [_vp, _double]),
    "lom_host_comm_abort": (_int, [_vp]),
    "lom_host_comm_allgather": (_int, [_vp, _vp, _size, _vp]),
    "lom_comm_attach_host": (_int, [_vp, _vp]),
    "lom_comm_attach_p2p": (_int, [_vp, _vp]),
    "lom_align_with_hooks": (_int, [_P(AlignHooks), _fp, _fp, _fp, _fp, _P(AlignStats)]),
    # ---- the stages before the align on the host, and the front end
    "lom_point_time_normalize": (None, [_vp, _size, _vp]),
    "lom_transform_non_rigid": (None, [_vp, _size, _pp, _pp, _vp]),
    "lom_range_filter": (_size, [_vp, _vp, _size, _float, _float, _vp, _vp]),
    "lom_cloud_classify": (_size, [_vp, _size, _vp, _vp, _P(_size), _P(_size)]),
    **_family("frontend", [_int, _vp]),
    "lom_frontend_set_option": (_int, _OPTION),
    "lom_frontend_process": (_int, [_vp, _vp, _size, _pp, _pp, _float, _float]),
    "lom_frontend_results": (_int, [_vp, _P(_vp), _P(_vp), _P(_vp), _P(_u32)]),
    "lom_frontend_deskewed": (_int, [_vp, _P(_vp), _P(_u32)]),
    "lom_frontend_wait": (_int, [_vp, _P(_u32)]),
    "lom_frontend_fetch": (_i64, [_vp, _int, _vp, _vp, _size]),
    "lom_frontend_stage": (_int, [_vp, _size, _P(_vp)]),
    "lom_frontend_done_event": (_vp, [_vp]),
    "lom_frontend_stream": (_vp, [_vp]),
    "lom_frontend_sequence": (_u32, [_vp]),
    "lom_debug_sinf": (_int, [_vp, _vp, _size, _vp]),
    "lom_classify_neighbourhood": (_i64, [_vp, _vp, _size, _P(NeighbourhoodParams), _vp, _vp, _vp]),
    "lom_frontend_set_classifier": (_int, _CLASSIFIER),
    "lom_frontend_debug_counter": (_i64, [_vp, _int]),
    # ---- files and messages
    "lom_pcd_read": (_i64, [_str, _vp, _vp, _size, _P(PcdInfo)]),
    "lom_pcd_last_error": (_str, []),
    "lom_pointcloud2_unpack": (_i64, [_P(Pc2View), _vp, _size, _P(_u32)]),
    "lom_pointcloud2_layout": (_int, [_int, _P(Pc2Field), _P(_u32)]),
    "lom_pointcloud2_pack_xyz": (_i64, [_vp, _size, _size, _vp, _size]),
    "lom_pointcloud2_last_error": (_str, []),
    "lom_estimate_normals": (_i64, [_vp, _size, _size, _float, _int, _vp, _vp]),
    # ---- place recognition
    **_family("place_db", [_P(PlaceParams), _int, _size]),
    "lom_place_db_size": (_i64, [_vp]),
    "lom_place_db_clear": (_int, [_vp]),
    "lom_place_db_params": (_int, [_vp, _P(PlaceParams)]),
    "lom_place_db_stream": (_vp, [_vp]),
    "lom_place_db_device": (_int, [_vp]),
    "lom_place_db_wait_event": (_int, [_vp, _vp]),
    "lom_place_describe": (_int, _DESCRIBE),
    "lom_place_describe_device": (_int, _DESCRIBE),
    "lom_place_db_add": (_i64, [_vp, _vp]),
    "lom_place_db_add_cloud": (_i64, _ADD_CLOUD),
    "lom_place_db_add_cloud_device": (_i64, _ADD_CLOUD),
    "lom_place_db_get": (_int, [_vp, _i64, _vp]),
    "lom_place_db_query": (_int, [_vp, _vp, _int, _i64, _i64, _int, _vp, _vp]),
    "lom_place_db_query_cloud_device": (_int, [_vp, _vp, _size, _size, _i64, _i64, _int, _vp]),
    "lom_place_shift_yaw": (_double, [_P(PlaceParams), _u32]),
    # ---- pose graph
    **_family("graph", [_int, _size, _size]),
    "lom_graph_clear": (_int, [_vp]),
    "lom_graph_stream": (_vp, [_vp]),
    "lom_graph_device": (_int, [_vp]),
    "lom_graph_add_node": (_i64, [_vp, _vp, _int]),
    "lom_graph_add_nodes": (_i64, [_vp, _vp, _vp, _size]),
    "lom_graph_add_edge": (_i64, [_vp, _i64, _i64, _vp, _vp, _double]),
    "lom_graph_add_edges": (_i64, [_vp, _vp, _vp, _vp, _vp, _size]),
    "lom_graph_node_count": (_i64, [_vp]),
    "lom_graph_edge_count": (_i64, [_vp]),
    "lom_graph_get_poses": (_int, [_vp, _i64, _i64, _vp]),
    "lom_graph_set_pose": (_int, [_vp, _i64, _vp]),
    "lom_graph_set_fixed": (_int, [_vp, _i64, _int]),
    "lom_graph_optimize": (_int, [_vp, _P(GraphParams), _P(GraphStats)]),
    "lom_graph_evaluate": (_int, [_vp, _double, _vp, _vp, _vp, _vp, _vp]),
    "lom_graph_debug_matvec": (_int, [_vp, _double, _vp, _vp]),
    "lom_graph_edge_chi2": (_int, [_vp, _i64, _i64, _vp]),
    "lom_graph_check_gauge": (_int, [_i64, _vp, _i64, _vp, _P(_i64)]),
    "lom_graph_lm_policy": (_int, [_double, _double, _double, _dp, _dp, _dp]),
    "lom_graph_information_from_quality": (_int, [_P(QualityReport), _int, _vp]),
    "lom_graph_pose_from_f32": (_int, [_pp, _vp]),
    "lom_graph_pose_to_f32": (_int, [_vp, _pp]),
    # ---- scan archive, map assembly, scan votes
    **_family("archive", [_int, _size, _size]),
    "lom_archive_clear": (_int, [_vp]),
    "lom_archive_stream": (_vp, [_vp]),
    "lom_archive_device": (_int, [_vp]),
    "lom_archive_wait_event": (_int, [_vp, _vp]),
    "lom_archive_add": (_i64, _ADD),
    "lom_archive_add_device": (_i64, [*_ADD, _vp]),
    "lom_archive_scan_count": (_i64, [_vp]),
    "lom_archive_point_count": (_i64, [_vp]),
    "lom_archive_scan_size": (_i64, [_vp, _i64]),
    "lom_archive_get": (_i64, [_vp, _i64, _vp, _vp, _size]),
    "lom_map_assemble": (_int, [_vp, _vp, _vp, _vp, _size, _P(AssembleParams), _P(AssembleStats)]),
    "lom_graph_pose_rotation_matrix": (_int, [_vp, _vp]),
    "lom_map_carve_scans": (_int, [_vp, _vp, _vp, _vp, _size, _P(VoteParams), _P(VoteStats)]),
    "lom_map_scan_votes": (_i64, [_vp, _vp, _vp, _vp, _size, _P(VoteParams), _vp, _vp, _size]),
    "lom_archive_add_points": (_i64, _ADD_CLOUD),
    "lom_archive_add_points_device": (_i64, [*_ADD_CLOUD, _vp]),
    # ---- occupancy grid
    **_grid_family("occupancy", OccupancyGeometry),
    "lom_occupancy_integrate": (_int, [_vp, _vp, _vp, _vp, _size, _P(OccupancyRayParams), _P(OccupancyStats)]),
    "lom_occupancy_integrate_cloud": (_int, [_vp, _vp, _size, _size, _vp, _P(OccupancyRayParams), _P(OccupancyStats)]),
    "lom_occupancy_integrate_cloud_device": (_int, [_vp, _vp, _size, _size, _vp, _P(OccupancyRayParams), _vp, _P(OccupancyStats)]),
    "lom_occupancy_counts": (_i64, [_vp, _vp, _vp, _size]),
    "lom_occupancy_classify": (_int, [_vp, _P(OccupancyRule), _vp, _size, _P(OccupancySummary)]),
    "lom_occupancy_classify_device": (_int, [_vp, _P(OccupancyRule), _P(_vp)]),
    # ---- elevation grid
    **_grid_family("elevation", ElevationGeometry),
    "lom_elevation_integrate": (_int, [_vp, _vp, _vp, _vp, _size, _P(ElevationPointParams), _P(ElevationStats)]),
    "lom_elevation_integrate_cloud": (_int, [_vp, _vp, _size, _size, _vp, _P(ElevationPointParams), _P(ElevationStats)]),
    "lom_elevation_integrate_cloud_device": (_int, [_vp, _vp, _size, _size, _vp, _P(ElevationPointParams), _vp, _P(ElevationStats)]),
    "lom_elevation_cells": (_i64, [_vp, _vp, _vp, _vp, _vp, _size]),
    "lom_elevation_layers": (_int, [_vp, _P(ElevationLayerParams), _vp, _vp, _vp, _vp, _vp, _vp, _size]),
    "lom_elevation_cost": (_int, [_vp, _P(ElevationLayerParams), _P(ElevationCostParams), _vp, _size, _P(ElevationSummary)]),
    "lom_elevation_cost_device": (_int, [_vp, _P(ElevationLayerParams), _P(ElevationCostParams), _P(_vp)]),
    # ---- clearance grid
    **_grid_family("clearance", OccupancyGeometry),
    "lom_clearance_update": (_int, [_vp, _vp, _vp, _P(ClearanceParams), _P(ClearanceWindow), _P(ClearanceSummary)]),
    "lom_clearance_update_device": (_int, [_vp, _vp, _vp, _vp, _P(ClearanceParams), _P(ClearanceWindow), _P(ClearanceSummary)]),
    "lom_clearance_update_from_grids": (_int, [_vp, _vp, _P(OccupancyRule), _vp, _P(ElevationLayerParams), _P(ElevationCostParams),
                                               _P(ClearanceParams), _P(ClearanceWindow), _P(ClearanceSummary)]),
    "lom_clearance_cost": (_int, [_vp, _vp, _size, _P(ClearanceSummary)]),
    "lom_clearance_cost_device": (_int, [_vp, _P(_vp)]),
    "lom_clearance_distance_sq": (_int, [_vp, _vp, _size]),
    "lom_clearance_distance": (_int, [_vp, _vp, _size]),
    "lom_clearance_cost_table": (_i64, [_P(ClearanceParams), _P(OccupancyGeometry), _vp, _size]),
    "lom_clearance_query": (_int, [_vp, _vp, _size, _vp, _vp]),
    # ---- navigation field
    **_grid_family("navfield", OccupancyGeometry),
    "lom_navfield_solve": (_int, [_vp, _vp, _P(NavFieldParams), _int, _vp, _size, _P(NavFieldSummary)]),
    "lom_navfield_solve_device": (_int, [_vp, _vp, _vp, _P(NavFieldParams), _int, _vp, _size, _P(NavFieldSummary)]),
    "lom_navfield_solve_from_clearance": (_int, [_vp, _vp, _P(NavFieldParams), _int, _vp, _size, _P(NavFieldSummary)]),
    "lom_navfield_resolve": (_int, [_vp, _vp, _P(ClearanceWindow), _P(NavFieldSummary)]),
    "lom_navfield_resolve_device": (_int, [_vp, _vp, _vp, _P(ClearanceWindow), _P(NavFieldSummary)]),
    "lom_navfield_resolve_from_clearance": (_int, [_vp, _vp, _P(ClearanceWindow), _P(NavFieldSummary)]),
    "lom_navfield_resolve_stats": (_int, [_vp, _P(NavFieldResolveCounters)]),
    "lom_navfield_shift_resolve": (_int, [_vp, C.c_int32, C.c_int32, _vp, _P(ClearanceWindow), _P(NavFieldSummary)]),
    "lom_navfield_shift_resolve_device": (_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _P(ClearanceWindow), _P(NavFieldSummary)]),
    "lom_navfield_shift_resolve_from_clearance": (_int, [_vp, C.c_int32, C.c_int32, _vp, _P(ClearanceWindow), _P(NavFieldSummary)]),
    "lom_navfield_shift_stats": (_int, [_vp, _P(NavFieldShiftCounters)]),
    "lom_navfield_potential": (_int, [_vp, _vp, _size]),
    "lom_navfield_potential_device": (_int, [_vp, _P(_vp)]),
    "lom_navfield_paths": (_int, [_vp, _int, _vp, _size, _vp, _size, _vp]),
    "lom_navfield_query": (_int, [_vp, _vp, _size, _vp]),
    "lom_navfield_visible": (_int, [_vp, _vp, _size, _u32, _vp]),
    "lom_navfield_waypoints": (_int, [_vp, _int, _vp, _size, _P(NavFieldWaypointParams), _vp, _size, _vp, _vp]),
    "lom_navfield_cell_costs": (_int, [_P(NavFieldParams), _vp]),
    "lom_navfield_stats": (_int, [_vp, _P(NavFieldSolveStats)]),
    "lom_navfield_adopt": (_int, [_vp, _vp, _size, _P(NavFieldSummary)]),
    **_grid_family("navset", OccupancyGeometry),
    "lom_navset_create": (_int, [_P(OccupancyGeometry), _int, _size, _P(_vp)]),
    "lom_navset_field_count": (_size, [_vp]),
    "lom_navset_solve": (_int, [_vp, _vp, _P(NavFieldParams), _int, _vp, _vp, _size, _P(NavFieldSummary)]),
    "lom_navset_solve_device": (_int, [_vp, _vp, _vp, _P(NavFieldParams), _int, _vp, _vp, _size, _P(NavFieldSummary)]),
    "lom_navset_solve_from_clearance": (_int, [_vp, _vp, _P(NavFieldParams), _int, _vp, _vp, _size, _P(NavFieldSummary)]),
    "lom_navset_potential": (_int, [_vp, _size, _vp, _size]),
    "lom_navset_potential_device": (_int, [_vp, _size, _P(_vp)]),
    "lom_navset_gather": (_int, [_vp, _int, _vp, _size, _vp]),
    "lom_navset_nearest": (_int, [_vp, _vp, _vp, _vp]),
    "lom_navset_paths": (_int, [_vp, _vp, _int, _vp, _size, _vp, _size, _vp]),
    "lom_navset_stats": (_int, [_vp, _P(NavSetSolveStats)]),
    # ---- pose field
    **_grid_family("posefield", OccupancyGeometry),
    "lom_posefield_solve": (_int, [_vp, _vp, _P(PoseFieldParams), _vp, _size, _vp, _size, _P(PoseFieldSummary)]),
    "lom_posefield_solve_device": (_int, [_vp, _vp, _vp, _P(PoseFieldParams), _vp, _size, _vp, _size, _P(PoseFieldSummary)]),
    "lom_posefield_solve_from_clearance": (_int, [_vp, _vp, _P(PoseFieldParams), _vp, _size, _vp, _size, _P(PoseFieldSummary)]),
    "lom_posefield_resolve": (_int, [_vp, _vp, _P(ClearanceWindow), _P(PoseFieldSummary)]),
    "lom_posefield_resolve_device": (_int, [_vp, _vp, _vp, _P(ClearanceWindow), _P(PoseFieldSummary)]),
    "lom_posefield_resolve_from_clearance": (_int, [_vp, _vp, _P(ClearanceWindow), _P(PoseFieldSummary)]),
    "lom_posefield_resolve_stats": (_int, [_vp, _P(PoseFieldResolveCounters)]),
    "lom_posefield_potential": (_int, [_vp, _vp, _size]),
    "lom_posefield_potential_device": (_int, [_vp, _P(_vp)]),
    "lom_posefield_layers": (_int, [_vp, _vp, _size]),
    "lom_posefield_floor": (_int, [_vp, _vp, _vp, _size]),
    "lom_posefield_floor_device": (_int, [_vp, _P(_vp), _P(_vp)]),
    "lom_posefield_paths": (_int, [_vp, _vp, _size, _vp, _size, _vp]),
    "lom_posefield_query": (_int, [_vp, _vp, _vp, _size, _vp]),
    "lom_posefield_stats": (_int, [_vp, _P(PoseFieldSolveStats)]),
    "lom_posefield_stencils": (_int, [_vp, _size, _vp, _size, _vp]),
    "lom_posefield_heading_of_angle": (_u32, [_u32]),
    # ---- frontier regions
    **_grid_family("regions", OccupancyGeometry),
    "lom_regions_extract": (_int, [_vp, _vp, _vp, _vp, _P(RegionsParams), _P(RegionsSummary)]),
    "lom_regions_extract_device": (_int, [_vp, _vp, _vp, _vp, _vp, _P(RegionsParams), _P(RegionsSummary)]),
    "lom_regions_extract_from_grids": (_int, [_vp, _vp, _P(OccupancyRule), _vp, _vp, _P(RegionsParams), _P(RegionsSummary)]),
    "lom_regions_labels": (_int, [_vp, _vp, _size]),
    "lom_regions_labels_device": (_int, [_vp, _P(_vp)]),
    "lom_regions_list": (_int, [_vp, _vp, _size, _P(_size)]),
    "lom_regions_goals": (_int, [_vp, _int, _vp, _size, _P(_size)]),
    "lom_regions_query": (_int, [_vp, _vp, _size, _vp]),
    "lom_regions_stats": (_int, [_vp, _P(RegionsExtractStats)]),
    # ---- visibility grid
    **_grid_family("visibility", OccupancyGeometry),
    "lom_visibility_table": (_int, [_u32, _vp]),
    "lom_visibility_cast": (_int, [_vp, _vp, _vp, _size, _P(VisibilityParams), _P(VisibilitySummary)]),
    "lom_visibility_cast_device": (_int, [_vp, _vp, _vp, _vp, _size, _P(VisibilityParams), _P(VisibilitySummary)]),
    "lom_visibility_cast_from_occupancy": (_int, [_vp, _vp, _P(OccupancyRule), _vp, _size, _P(VisibilityParams), _P(VisibilitySummary)]),
    "lom_visibility_records": (_int, [_vp, _vp, _size, _P(_size)]),
    "lom_visibility_beams": (_int, [_vp, _vp, _size]),
    "lom_visibility_windows_device": (_int, [_vp, _P(_vp), _P(_size)]),
    "lom_visibility_windows": (_int, [_vp, _vp, _size, _P(_size)]),
    "lom_visibility_select": (_int, [_vp, _P(VisibilitySelectParams), _vp, _vp, _P(_size)]),
    "lom_visibility_select_from_navfield": (_int, [_vp, _vp, _P(VisibilitySelectParams), _vp, _P(_size)]),
    "lom_visibility_stats": (_int, [_vp, _P(VisibilityCallStats)]),
    # ---- trajectory rollouts
    **_grid_family("rollout", OccupancyGeometry),
    "lom_rollout_evaluate": (_int, [_vp, _vp, _vp] + _ROLLOUT_TAIL),
    "lom_rollout_evaluate_device": (_int, [_vp, _vp, _vp, _vp, _vp] + _ROLLOUT_TAIL),
    "lom_rollout_evaluate_from_grids": (_int, [_vp, _vp, _vp] + _ROLLOUT_TAIL),
    "lom_rollout_records": (_int, [_vp, _vp, _size, _P(_size)]),
    "lom_rollout_stats": (_int, [_vp, _P(RolloutCallStats)]),
    "lom_rollout_footprint_rectangle": (_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _int, _vp, _size, _P(_size)]),
    "lom_rollout_state_from_pose": (_int, [_P(OccupancyGeometry), _float, _float, _float, _vp]),
    "lom_rollout_poses": (_int, [_P(RolloutParams), _vp, _vp, _vp]),
    # ---- grid shift (the families' own lom_<stem>_shift: _grid_family)
    "lom_grid_shift_geometry": (_int, [_P(OccupancyGeometry), C.c_int32, C.c_int32, _P(OccupancyGeometry)]),
    "lom_grid_follow": (_int, [_P(OccupancyGeometry), _double, _double, _u32, _u32, _P(C.c_int32), _P(C.c_int32)]),
    # ---- the odometry
    "lom_odometry_default_params": (None, [_P(OdometryParams)]),
    **_family("odometry", [_P(OdometryParams), _int]),
    "lom_odometry_process_cloud": (_int, [_vp, _vp, _size]),
    "lom_odometry_process_sequence": (_int, [_vp, _P(_vp), _P(_size), _size, _P(_size)]),
    "lom_odometry_process_batch": (_int, [_P(_vp), _P(_vp), _P(_size), _int, _P(_int)]),
    "lom_odometry_hint_next": (_int, [_vp, _vp, _size]),
    "lom_odometry_get_pose": (_int, [_vp, _pp]),
    "lom_odometry_get_temp_cloud": (_i64, [_vp, _vp, _size]),
    "lom_odometry_place_descriptor": (_int, [_vp, _vp, _int, _vp, _P(_i64)]),
    "lom_odometry_archive_scan": (_int, [_vp, _vp, _P(_i64)]),
    "lom_odometry_archive_deskewed": (_int, [_vp, _vp, _P(_i64)]),
    "lom_odometry_occupancy_scan": (_int, [_vp, _vp, _P(OccupancyRayParams), _P(OccupancyStats)]),
    "lom_odometry_elevation_scan": (_int, [_vp, _vp, _P(ElevationPointParams), _P(ElevationStats)]),
    "lom_odometry_rebuild_keyframe": (_int, [_vp, _vp, _vp, _vp, _size, _pp, _P(AssembleStats)]),
    "lom_odometry_get_stats": (_int, [_vp, _P(OdometryFrameStats)]),
    "lom_odometry_set_quality_thresholds": (_int, [_vp, _float, _float]),
    "lom_odometry_get_quality": (_int, [_vp, _P(QualityReport)]),
    "lom_odometry_set_option": (_int, _OPTION),
    "lom_odometry_set_classifier": (_int, _CLASSIFIER),
    "lom_odometry_set_carve": (_int, [_vp, _P(CarveParams)]),
    "lom_odometry_get_carve_stats": (_int, [_vp, _P(CarveStats)]),
    "lom_odometry_set_rebuild_votes": (_int, [_vp, _P(VoteParams)]),
    "lom_odometry_get_rebuild_vote_stats": (_int, [_vp, _P(VoteStats)]),
    "lom_odometry_debug_counter": (_i64, [_vp, _int]),
    "lom_odometry_debug_set_state": (_int, [_vp, _pp, _pp]),
    "lom_odometry_keyframe": (_vp, [_vp]),
}
# the one function the header declares through a function type (the "scan archive and map assembly" section) ...
EXPORTED_BY_TYPE = ["lom_graph_pose_rotation_matrix"]
# ... and the two of the same section that came with the occupancy grid, declared the same way
EXPORTED_BY_TYPE_POINTS = ["lom_archive_add_points", "lom_archive_add_points_device"]
# ... and the seven shifts of the "grid shift" section, one per grid family, declared the same way
EXPORTED_BY_TYPE_SHIFT = [f"lom_{stem}_shift" for stem in ("occupancy", "elevation", "clearance", "navfield", "regions", "visibility", "rollout")]
# every symbol include/lidar_odometry_amd.h declares with its parameters
EXPORTED = [name for name in PROTOTYPES if name not in EXPORTED_BY_TYPE + EXPORTED_BY_TYPE_POINTS + EXPORTED_BY_TYPE_SHIFT]

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
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
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
