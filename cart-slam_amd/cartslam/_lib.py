"""ctypes binding of the C ABI declared in include/cart_engine.h.

The shared library is built in-tree by `make -C cart-slam_amd` (or __graft_entry__.build()).
There is NO fallback: if the library is missing, loading raises and every op fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CART_ENGINE_LIB") or os.path.join(os.path.dirname(_HERE), "build", "libcart_engine.so")  # override: timing experiments


class EngineParams(C.Structure):
    # mirrors cart_engine_params (include/cart_engine.h)
    _fields_ = [(n, C.c_int) for n in (
        "device_id", "width", "height", "min_disparity", "num_disparities", "paths", "p1", "p2",
        "uniqueness_ratio", "smoothing_radius", "smoothing_iterations", "max_inflight")]


class PlaneParams(C.Structure):
    # mirrors cart_plane_params (include/cart_engine.h; reference include/modules/planeseg.hpp:25-34)
    _fields_ = [(n, C.c_int) for n in (
        "horizontal_min", "horizontal_max", "vertical_min", "vertical_max",
        "horizontal_center", "vertical_center")]

    def as_tuple(self):
        return tuple(getattr(self, n) for n, _ in self._fields_)


class LaunchPlan(C.Structure):
    # mirrors cart_launch_plan (include/cart_engine.h)
    _fields_ = [("frames_per_launch", C.c_int), ("plan", C.c_int), ("slabs_written", C.c_int)]


PLAN_AUTO, PLAN_SLABS, PLAN_FUSED_UP, PLAN_BAND_UP = -1, 0, 1, 2      # CART_PLAN_*
OPT_PLAN, OPT_PLAN_MIN_FRAMES, OPT_CHUNK_FRAMES = 0, 1, 2           # CART_OPT_*
OPT_BAND_ROWS, OPT_BAND_PROBE = 6, 7
OPT_BAND_DIAG = 9
OPT_FLOW_GATHER = 8
OPT_SPEC_S8_ZERO_INVALID, OPT_SPEC_S7_REPLICATE_BORDER, OPT_SPEC_S5_TOP2 = 3, 4, 5   # CART_OPT_SPEC_*: upstream variants of oracle S8 / S7 / S5


class FlowParams(C.Structure):
    # mirrors cart_flow_params (include/cart_engine.h, spec S21)
    _fields_ = [(n, C.c_int) for n in ("levels", "radius", "refine_radius", "block", "median")]


FLOW_MAX_LEVELS = 6


class PlacementReport(C.Structure):
    # mirrors cart_placement_report (include/cart_engine.h)
    _fields_ = [("ms_first", C.c_float), ("ms_kept", C.c_float), ("ms_fastest_seen", C.c_float), ("ms_slowest_seen", C.c_float),
                ("seconds", C.c_float), ("units", C.c_int), ("candidates", C.c_int), ("mode", C.c_int), ("stop_reason", C.c_int)]


PRED_PLANEFIT, PRED_PLANECLUSTER = 0, 1        # CART_PLANE_PREDICATE_*
PLANEFIT_MAX_PLANES = 100                      # CART_PLANEFIT_MAX_PLANES
PLANEFIT_THRESHOLD = 0.01                      # CART_PLANEFIT_THRESHOLD


ORB_DEFAULT_FEATURES, ORB_MAX_FEATURES, ORB_LEVELS, ORB_DESCRIPTOR_BYTES = 5000, 65536, 8, 32   # CART_ORB_*


class Keypoint(C.Structure):
    # mirrors cart_keypoint (include/cart_engine.h): cv::KeyPoint's layout
    _fields_ = [(n, C.c_float) for n in ("x", "y", "size", "angle", "response")] + [("octave", C.c_int32), ("class_id", C.c_int32)]


class Match(C.Structure):
    # mirrors cart_match (include/cart_engine.h, spec S22)
    _fields_ = [(n, C.c_int32) for n in ("query", "train", "distance", "second")]


class MatchParams(C.Structure):
    # mirrors cart_match_params (include/cart_engine.h, spec S22); the defaults are cart_match_default_params'
    _fields_ = [("use_gate", C.c_int32)] + [(n, C.c_float) for n in ("dx_min", "dx_max", "dy_min", "dy_max")] + \
               [(n, C.c_int32) for n in ("max_octave_diff", "max_distance", "ratio", "cross_check")]


class EgoCamera(C.Structure):
    # mirrors cart_ego_camera (include/cart_engine.h, spec S23)
    _fields_ = [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "baseline")]


class EgoParams(C.Structure):
    # mirrors cart_ego_params (include/cart_engine.h, spec S23); the defaults are cart_ego_default_params'
    _fields_ = [("min_disparity", C.c_double), ("inlier_threshold", C.c_double), ("hypotheses", C.c_int32), ("refine_iterations", C.c_int32)]


class EgoResult(C.Structure):
    # mirrors cart_ego_result (include/cart_engine.h, spec S23)
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("rms", C.c_double)] + \
               [(n, C.c_int32) for n in ("status", "n_correspondences", "n_inliers", "best_hypothesis")]


class EgoHypothesis(C.Structure):
    # mirrors cart_ego_hypothesis (include/cart_engine.h, spec S23)
    _fields_ = [("qerr", C.c_uint64), ("count", C.c_int32), ("skipped", C.c_int32)]


EGO_MAX_HYPOTHESES, EGO_MAX_REFINE = 1024, 16   # CART_EGO_MAX_*


class PlaneMapParams(C.Structure):
    # mirrors cart_plane_map_params (include/cart_engine.h, spec S24); the defaults are cart_plane_map_default_params'
    _fields_ = [(n, C.c_double) for n in ("cell_size", "min_disparity", "max_depth", "max_lateral", "height_quantum")]


class PlaneMapCell(C.Structure):
    # mirrors cart_plane_map_cell (include/cart_engine.h, spec S24)
    _fields_ = [("horizontal", C.c_uint32), ("vertical", C.c_uint32), ("y_min", C.c_int32), ("y_max", C.c_int32)]


class MotionParams(C.Structure):
    # mirrors cart_motion_params (include/cart_engine.h, spec S25); the defaults are cart_motion_default_params'
    _fields_ = [(n, C.c_double) for n in ("min_disparity", "flow_threshold", "disparity_threshold")] + [(n, C.c_int32) for n in ("radius", "support_percent")]


class DenseEgoParams(C.Structure):
    # mirrors cart_dense_ego_params (include/cart_engine.h, spec S26); the defaults are cart_dense_ego_default_params'
    _fields_ = [(n, C.c_double) for n in ("min_disparity", "flow_threshold", "disparity_threshold", "disparity_weight")] + \
               [(n, C.c_int32) for n in ("iterations", "stride", "min_inliers")]


class PlaceParams(C.Structure):
    # mirrors cart_place_params (include/cart_engine.h, spec S27); the defaults are cart_place_default_params'
    _fields_ = [(n, C.c_int32) for n in ("max_distance", "ratio", "min_score", "max_candidates")] + [("min_gap", C.c_uint64)]


class PlaceCandidate(C.Structure):
    # mirrors cart_place_candidate (include/cart_engine.h, spec S27)
    _fields_ = [("slot", C.c_int32), ("score", C.c_int32), ("frame_id", C.c_uint64)]


class DenseEgoResult(C.Structure):
    # mirrors cart_dense_ego_result (include/cart_engine.h, spec S26)
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("rms_initial", C.c_double), ("rms", C.c_double)] + \
               [(n, C.c_int32) for n in ("status", "n_candidates", "n_initial", "n_inliers", "steps", "reserved")]


DENSE_EGO_MAX_ITERATIONS = 16   # CART_DENSE_EGO_MAX_ITERATIONS


class FusionParams(C.Structure):
    # mirrors cart_fusion_params (include/cart_engine.h, spec S28); the defaults are cart_fusion_default_params' (build-owned, untuned)
    _fields_ = [(n, C.c_double) for n in ("min_disparity", "agree_threshold", "splat_radius")] + [(n, C.c_int32) for n in ("max_weight", "min_age")]


class PoseGraphParams(C.Structure):
    # mirrors cart_pose_graph_params (include/cart_engine.h, spec S29); the default is cart_pose_graph_default_params'
    _fields_ = [("iterations", C.c_int32)]


class PoseGraphResult(C.Structure):
    # mirrors cart_pose_graph_result (include/cart_engine.h, spec S29)
    _fields_ = [(n, C.c_int32) for n in ("status", "n_nodes", "n_loops", "iterations")] + [("cost_before", C.c_double), ("cost_after", C.c_double)]


POSE_GRAPH_MAX_NODES, POSE_GRAPH_MAX_LOOPS, POSE_GRAPH_MAX_ITERATIONS = 4096, 64, 16   # CART_POSE_GRAPH_MAX_*


class LocalBAParams(C.Structure):
    # mirrors cart_local_ba_params (include/cart_engine.h, spec S32); the defaults are cart_local_ba_default_params' (build-owned, untuned)
    _fields_ = [(n, C.c_double) for n in ("min_disparity", "huber", "damping")] + [(n, C.c_int32) for n in ("iterations", "min_observations", "min_frame_observations")]


class LocalBAResult(C.Structure):
    # mirrors cart_local_ba_result (include/cart_engine.h, spec S32)
    _fields_ = [(n, C.c_int32) for n in ("status", "n_frames", "n_points_active", "n_observations", "n_held", "iterations")] + \
               [("cost_before", C.c_double), ("cost_after", C.c_double)]


LOCAL_BA_MAX_WINDOW, LOCAL_BA_MAX_POINTS, LOCAL_BA_MAX_ITERATIONS = 16, 65536, 16   # CART_LOCAL_BA_MAX_*


class ObjectParams(C.Structure):
    # mirrors cart_object_params (include/cart_engine.h, spec S31); the defaults are cart_object_default_params' (build-owned, untuned)
    _fields_ = [(n, C.c_double) for n in ("min_disparity", "disparity_band", "max_speed", "gate")] + \
               [(n, C.c_int32) for n in ("min_area", "min_points", "gain_percent", "max_missed", "min_age")]


class Object(C.Structure):
    # mirrors cart_object (include/cart_engine.h, spec S31)
    _fields_ = [(n, C.c_int32) for n in ("component", "area", "x0", "y0", "x1", "y1", "median_bin", "n_hist", "n_points", "n_flow")] + \
               [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("sum", C.c_int64 * 3), ("flow_sum", C.c_int64 * 3), ("centroid", C.c_double * 3),
                ("velocity", C.c_double * 3), ("extent", C.c_double * 3), ("valid", C.c_int32), ("has_velocity", C.c_int32)]


class Track(C.Structure):
    # mirrors cart_track (include/cart_engine.h, spec S31)
    _fields_ = [("id", C.c_uint32)] + [(n, C.c_int32) for n in ("state", "age", "missed", "object", "component")] + \
               [("position", C.c_double * 3), ("velocity", C.c_double * 3), ("extent", C.c_double * 3)]


OBJECT_BINS, OBJECT_MAX_OBJECTS, OBJECT_MAX_TRACKS = 512, 256, 256   # CART_OBJECT_*


class VoxelMapParams(C.Structure):
    # mirrors cart_voxel_map_params (include/cart_engine.h, spec S33); the defaults are cart_voxel_map_default_params' (build-owned, untuned)
    _fields_ = [(n, C.c_double) for n in ("voxel_size", "min_disparity", "min_depth", "max_depth", "truncation", "disparity_sigma", "lookahead", "march_step")] + \
               [(n, C.c_int32) for n in ("max_weight", "min_weight")]


class Voxel(C.Structure):
    # mirrors cart_voxel (include/cart_engine.h, spec S33)
    _fields_ = [("tsdf", C.c_int16), ("weight", C.c_uint16)]


class VoxelRgb(C.Structure):
    # mirrors cart_voxel_rgb (include/cart_engine.h, spec S37)
    _fields_ = [("b", C.c_uint8), ("g", C.c_uint8), ("r", C.c_uint8), ("weight", C.c_uint8)]


VOXEL_COLOR_DEFAULT_MAX_WEIGHT = 64   # CART_VOXEL_COLOR_DEFAULT_MAX_WEIGHT (build-owned, untuned)
VOXEL_RAY_NONE, VOXEL_RAY_HIT, VOXEL_RAY_INSIDE = range(3)   # CART_VOXEL_RAY_*


class MeshVertex(C.Structure):
    # mirrors cart_mesh_vertex (include/cart_engine.h, spec S36)
    _fields_ = [("position", C.c_float * 3), ("normal", C.c_float * 3)]


class MeshQuad(C.Structure):
    # mirrors cart_mesh_quad (include/cart_engine.h, spec S36)
    _fields_ = [("v", C.c_int32 * 4)]


class ModelTrackParams(C.Structure):
    # mirrors cart_model_track_params (include/cart_engine.h, spec S34); the defaults are cart_model_track_default_params' (build-owned, untuned)
    _fields_ = [(n, C.c_double) for n in ("residual_gate", "damping")] + [(n, C.c_int32) for n in ("iterations", "stride", "min_inliers")]


class ModelTrackResult(C.Structure):
    # mirrors cart_model_track_result (include/cart_engine.h, spec S34): the layout of cart_dense_ego_result
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("rms_initial", C.c_double), ("rms", C.c_double)] + \
               [(n, C.c_int32) for n in ("status", "n_candidates", "n_initial", "n_inliers", "steps", "reserved")]


MODEL_TRACK_MAX_ITERATIONS = 16   # CART_MODEL_TRACK_MAX_ITERATIONS


class ModelTrackColorParams(C.Structure):
    # mirrors cart_model_track_color_params (include/cart_engine.h, spec S38); the defaults are cart_model_track_color_default_params' (build-owned, untuned)
    _fields_ = [(n, C.c_double) for n in ("photo_weight", "photo_gate")] + [(n, C.c_int32) for n in ("color_min_weight", "reserved")]


class ModelTrackColorResult(C.Structure):
    # mirrors cart_model_track_color_result (include/cart_engine.h, spec S38): cart_model_track_result, then the photometric figures
    _fields_ = ModelTrackResult._fields_ + [(n, C.c_double) for n in ("rms_photo_initial", "rms_photo", "cost_initial", "cost")] + \
               [(n, C.c_int32) for n in ("n_photo_initial", "n_photo")]


FUSION_NONE, FUSION_MEASURED, FUSION_AGREED, FUSION_REPLACED, FUSION_PREDICTED = range(5)   # CART_FUSION_*


PLACE_MODES = {0: "unknown", 1: "fast", 2: "mixed", 3: "uniform"}                                       # CART_PLACE_MODE_*
PLACE_STOPS = {0: "nothing to do", 1: "fast set found", 2: "uniform", 3: "tries", 4: "time", 5: "memory"}   # CART_PLACE_STOP_*


class SuperpixelParams(C.Structure):
    # mirrors cart_superpixel_params (include/cart_engine.h; reference cartconfig.cpp:121-133)
    _fields_ = [(n, C.c_double) for n in (
        "direct_clique_cost", "diagonal_clique_cost", "compactness_weight", "progressive_compactness_cost",
        "image_weight", "disparity_weight")]


# every symbol include/cart_engine.h declares, with its prototype
_vp, _sz, _i = C.c_void_p, C.c_size_t, C.c_int
PROTOTYPES = {
    "cart_engine_default_params": (None, [C.POINTER(EngineParams)]),
    "cart_engine_create": (_i, [C.POINTER(EngineParams), C.POINTER(_vp)]),
    "cart_engine_destroy": (None, [_vp]),
    "cart_last_error": (C.c_char_p, [_vp]),
    "cart_engine_set_option": (_i, [_vp, _i, _i]),
    "cart_engine_get_option": (_i, [_vp, _i, C.POINTER(_i)]),
    "cart_engine_describe_plan": (_i, [_vp, _i, C.POINTER(LaunchPlan)]),
    "cart_engine_tune_placement": (_i, [_vp, _i, _i, _sz, C.POINTER(PlacementReport)]),
    "cart_compute_disparity": (_i, [_vp, _vp, _sz, _vp, _sz, _i, _vp, _sz, _vp]),
    "cart_compute_disparity_batch": (_i, [_vp, _i, _vp, _sz, _sz, _vp, _sz, _sz, _i, _vp, _sz, _sz, _vp]),
    "cart_compute_disparity_multi": (_i, [_vp, _i, _vp, _sz, _vp, _sz, _i, _vp, _sz, _vp]),
    "cart_interpolate": (_i, [_vp, _i, _vp, _sz, _sz, _i, _i, _i, _i, _vp]),
    "cart_disparity_derivative": (_i, [_vp, _i, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _vp]),
    "cart_plane_derivative_hist": (_i, [_vp, _i, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _sz, _vp]),
    "cart_plane_classify": (_i, [_vp, _i, _vp, _sz, _sz, C.POINTER(PlaneParams), _i, _vp, _sz, _sz, _vp]),
    "cart_plane_derivative_hist_multi": (_i, [_vp, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "cart_plane_classify_multi": (_i, [_vp, _i, _vp, _sz, C.POINTER(PlaneParams), _i, _vp, _sz, _vp]),
    "cart_plane_ccl": (_i, [_vp, _i, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _vp]),
    "cart_plane_ccl_stats": (_i, [_vp, _i, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _i, _vp, _vp]),
    "cart_plane_ccl_table": (_i, [_vp, _i, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _i, _vp, _vp]),
    "cart_plane_schedule_create": (_i, [_vp, _i, C.POINTER(PlaneParams), _i, _i, C.POINTER(_vp)]),
    "cart_plane_schedule_destroy": (None, [_vp]),
    "cart_plane_schedule_advance": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "cart_plane_schedule_read": (_i, [_vp, C.POINTER(PlaneParams), C.POINTER(C.c_int32)]),
    "cart_plane_classify_dev": (_i, [_vp, _i, _vp, _sz, _sz, _vp, _i, _vp, _sz, _sz, _vp]),
    "cart_plane_temporal_vote": (_i, [_vp, _vp, _sz, _i, C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_vp), C.POINTER(_sz), _vp, _sz, _vp]),
    "cart_reproject_depth": (_i, [_vp, _i, _vp, _sz, _sz, C.POINTER(C.c_float), _vp, _sz, _sz, _vp]),
    "cart_superpixel_default_params": (None, [C.POINTER(SuperpixelParams)]),
    "cart_superpixels_create": (_i, [_vp, C.POINTER(SuperpixelParams), _i, _i, C.POINTER(_vp)]),
    "cart_superpixels_destroy": (None, [_vp]),
    "cart_superpixels_reset": (_i, [_vp, _vp]),
    "cart_superpixels_set_labels": (_i, [_vp, _vp, _sz, _i, _vp]),
    "cart_superpixels_relax": (_i, [_vp, _vp, _sz, _i, _vp, _sz, _i, _vp, _sz, _vp]),
    "cart_superpixels_max_label": (_i, [_vp]),
    "cart_superpixel_plane_classify": (_i, [_vp, _vp, _sz, _vp, _sz, _i, C.POINTER(PlaneParams), _i, C.POINTER(_vp), C.POINTER(_sz),
                                           C.POINTER(_vp), C.POINTER(_sz), _vp, _sz, _vp, _sz, _vp]),
    "cart_planefit_create": (_i, [_vp, _i, C.POINTER(_vp)]),
    "cart_planefit_destroy": (None, [_vp]),
    "cart_planefit_label_planes": (_i, [_vp, _vp, _sz, _i, _vp, _sz, _i, C.c_double, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _vp]),
    "cart_planefit_points": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "cart_planefit_adjacency": (_i, [_vp, _vp, _sz, _i, _vp, _vp, _sz, _vp]),
    "cart_planefit_fit": (_i, [_vp, _vp, _sz, C.c_uint64, C.c_uint64, _vp, _vp, _vp, C.POINTER(_i), _vp]),
    "cart_planefit_status": (_i, [_vp, C.POINTER(_i)]),
    "cart_plane_cluster": (_i, [_vp, _i, _vp, _vp, _vp, _vp, C.POINTER(_i)]),
    "cart_orb_create": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "cart_orb_destroy": (None, [_vp]),
    "cart_orb_levels": (_i, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "cart_orb_detect": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_sz), _i, _i, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_sz), _vp, _vp]),
    "cart_orb_debug_level": (_i, [_vp, _i, _i, _vp, _sz, C.POINTER(C.c_int32), _vp]),
    "cart_match_default_params": (None, [C.POINTER(MatchParams)]),
    "cart_matcher_create": (_i, [_vp, _i, C.POINTER(_vp)]),
    "cart_matcher_destroy": (None, [_vp]),
    "cart_matcher_match": (_i, [_vp, C.POINTER(MatchParams), _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cart_ego_default_params": (None, [C.POINTER(EgoParams)]),
    "cart_ego_create": (_i, [_vp, _i, C.POINTER(_vp)]),
    "cart_ego_destroy": (None, [_vp]),
    "cart_ego_triangulate": (_i, [_vp, C.POINTER(EgoCamera), C.POINTER(EgoParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cart_ego_estimate": (_i, [_vp, C.POINTER(EgoCamera), C.POINTER(EgoParams), _vp, _vp, _vp, _vp, _vp, C.c_uint64, C.c_uint64, _vp, _vp, _vp]),
    "cart_ego_debug_hypotheses": (_i, [_vp, C.POINTER(EgoHypothesis), _i, C.POINTER(_i), _vp]),
    "cart_plane_map_default_params": (None, [C.POINTER(PlaneMapParams)]),
    "cart_plane_map_create": (_i, [_vp, _i, _i, C.POINTER(PlaneMapParams), C.POINTER(_vp)]),
    "cart_plane_map_destroy": (None, [_vp]),
    "cart_plane_map_clear": (_i, [_vp]),
    "cart_plane_map_update": (_i, [_vp, C.POINTER(EgoCamera), C.POINTER(C.c_double), _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "cart_plane_map_window": (_i, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(_i)]),
    "cart_plane_map_read": (_i, [_vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _vp]),
    "cart_plane_map_classify": (_i, [_vp, _i, _i, _vp, _sz, _vp]),
    "cart_plane_store_create": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "cart_plane_store_destroy": (None, [_vp]),
    "cart_plane_store_clear": (_i, [_vp]),
    "cart_plane_store_size": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "cart_plane_store_insert": (_i, [_vp, C.c_uint64, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "cart_plane_store_contains": (_i, [_vp, C.c_uint64, C.POINTER(_i)]),
    "cart_plane_map_rebuild": (_i, [_vp, _vp, C.POINTER(EgoCamera), C.POINTER(C.c_uint64), C.POINTER(C.c_double), _i, C.POINTER(C.c_double), C.POINTER(_i), _vp]),
    "cart_motion_default_params": (None, [C.POINTER(MotionParams)]),
    "cart_motion_segment": (_i, [_vp, C.POINTER(EgoCamera), C.POINTER(C.c_double), C.POINTER(MotionParams), _vp, _sz, _vp, _sz, _vp, _sz, _i, _i,
                                 _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "cart_dense_ego_default_params": (None, [C.POINTER(DenseEgoParams)]),
    "cart_dense_ego_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "cart_dense_ego_destroy": (None, [_vp]),
    "cart_dense_ego_refine": (_i, [_vp, C.POINTER(EgoCamera), C.POINTER(C.c_double), C.POINTER(DenseEgoParams), _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz,
                                   _i, _i, _vp, _vp]),
    "cart_place_default_params": (None, [C.POINTER(PlaceParams)]),
    "cart_place_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "cart_place_destroy": (None, [_vp]),
    "cart_place_clear": (_i, [_vp, _vp]),
    "cart_place_insert": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, C.c_uint64, C.POINTER(C.c_int32), _vp]),
    "cart_place_query": (_i, [_vp, C.POINTER(PlaceParams), _vp, _sz, _vp, C.c_uint64, _vp, _vp, _vp, _vp]),
    "cart_place_slot": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "cart_fusion_default_params": (None, [C.POINTER(FusionParams)]),
    "cart_fusion_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "cart_fusion_destroy": (None, [_vp]),
    "cart_fusion_update": (_i, [_vp, C.POINTER(EgoCamera), C.POINTER(C.c_double), C.POINTER(FusionParams), _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz,
                                _i, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
    "cart_pose_graph_default_params": (None, [C.POINTER(PoseGraphParams)]),
    "cart_pose_graph_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "cart_pose_graph_destroy": (None, [_vp]),
    "cart_pose_graph_clear": (_i, [_vp, _vp]),
    "cart_pose_graph_size": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "cart_pose_graph_add_node": (_i, [_vp, C.POINTER(C.c_double), C.c_double, C.c_double, C.POINTER(C.c_int32), _vp]),
    "cart_pose_graph_add_loop": (_i, [_vp, _i, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double, _vp]),
    "cart_pose_graph_optimize": (_i, [_vp, C.POINTER(PoseGraphParams), _vp, _vp]),
    "cart_pose_graph_poses": (_i, [_vp, _i, _i, _vp, _vp]),
    "cart_pose_graph_read": (_i, [_vp, _i, _i, C.POINTER(C.c_double)]),
    "cart_object_default_params": (None, [C.POINTER(ObjectParams)]),
    "cart_object_tracker_create": (_i, [_vp, _i, _i, _i, _i, C.POINTER(_vp)]),
    "cart_object_tracker_destroy": (None, [_vp]),
    "cart_object_tracker_reset": (_i, [_vp, _vp]),
    "cart_object_tracker_update": (_i, [_vp, C.POINTER(EgoCamera), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(ObjectParams), _vp, _sz, _vp, _i, _vp,
                                        _vp, _sz, _vp, _sz, _vp, _sz, _i, _i, _vp, _vp, _vp, _vp]),
    "cart_local_ba_default_params": (None, [C.POINTER(LocalBAParams)]),
    "cart_local_ba_create": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "cart_local_ba_destroy": (None, [_vp]),
    "cart_local_ba_clear": (_i, [_vp, _vp]),
    "cart_local_ba_size": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "cart_local_ba_push": (_i, [_vp, C.POINTER(EgoCamera), C.POINTER(LocalBAParams), C.c_uint64, C.POINTER(C.c_double), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cart_local_ba_optimize": (_i, [_vp, C.POINTER(EgoCamera), C.POINTER(LocalBAParams), _vp, _vp]),
    "cart_local_ba_poses": (_i, [_vp, _vp, _vp, _vp]),
    "cart_local_ba_points": (_i, [_vp, _vp, _vp]),
    "cart_local_ba_track_of": (_i, [_vp, _vp, _vp]),
    "cart_voxel_map_default_params": (None, [C.POINTER(VoxelMapParams)]),
    "cart_voxel_map_create": (_i, [_vp, _i, _i, _i, C.POINTER(VoxelMapParams), C.POINTER(_vp)]),
    "cart_voxel_map_destroy": (None, [_vp]),
    "cart_voxel_map_clear": (_i, [_vp]),
    "cart_voxel_map_window": (_i, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(_i)]),
    "cart_voxel_map_integrate": (_i, [_vp, C.POINTER(EgoCamera), C.POINTER(C.c_double), _vp, _sz, _i, _i, _vp, _sz, _vp, _vp]),
    "cart_voxel_map_raycast": (_i, [_vp, C.POINTER(EgoCamera), C.POINTER(C.c_double), _i, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
    "cart_voxel_map_read": (_i, [_vp, _vp, C.POINTER(C.c_int64), _vp]),
    "cart_voxel_map_mesh": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, C.POINTER(C.c_int64), _vp]),
    "cart_voxel_map_write": (_i, [_vp, _vp, C.POINTER(C.c_int64), _vp]),
    "cart_voxel_map_rebuild": (_i, [_vp, _vp, C.POINTER(EgoCamera), C.POINTER(C.c_uint64), C.POINTER(C.c_double), _i, C.POINTER(C.c_double), _i, C.POINTER(_i), _vp, _vp]),
    "cart_voxel_color_create": (_i, [_vp, _vp, _i, C.POINTER(_vp)]),
    "cart_voxel_color_destroy": (None, [_vp]),
    "cart_voxel_color_clear": (_i, [_vp]),
    "cart_voxel_color_window": (_i, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(_i)]),
    "cart_voxel_color_integrate": (_i, [_vp, _vp, C.POINTER(EgoCamera), C.POINTER(C.c_double), _vp, _sz, _vp, _sz, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "cart_voxel_color_vertices": (_i, [_vp, _vp, _vp, _i, C.POINTER(C.c_int64), _vp, _vp]),
    "cart_voxel_color_render": (_i, [_vp, C.POINTER(EgoCamera), C.POINTER(C.c_double), _vp, _sz, _i, _i, _vp, _sz, _vp, _sz, _vp, _vp]),
    "cart_voxel_color_read": (_i, [_vp, _vp, C.POINTER(C.c_int64), _vp]),
    "cart_voxel_color_write": (_i, [_vp, _vp, C.POINTER(C.c_int64), _vp]),
    "cart_model_track_default_params": (None, [C.POINTER(ModelTrackParams)]),
    "cart_model_track_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "cart_model_track_destroy": (None, [_vp]),
    "cart_model_track_refine": (_i, [_vp, _vp, C.POINTER(EgoCamera), C.POINTER(C.c_double), C.POINTER(ModelTrackParams), _vp, _sz, _vp, _sz, _i, _i, _vp, _vp]),
    "cart_model_track_color_default_params": (None, [C.POINTER(ModelTrackColorParams)]),
    "cart_model_track_refine_color": (_i, [_vp, _vp, _vp, C.POINTER(EgoCamera), C.POINTER(C.c_double), C.POINTER(ModelTrackParams), C.POINTER(ModelTrackColorParams),
                                           _vp, _sz, _vp, _sz, _i, _vp, _sz, _i, _i, _vp, _vp]),
    "cart_optical_flow": (_i, [_vp, _vp, _sz, _vp, _sz, _i, _i, _i, _vp, _sz, _vp]),
    "cart_flow_default_params": (None, [C.POINTER(FlowParams)]),
    "cart_flow_pyramid_levels": (_i, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "cart_optical_flow_pyramid": (_i, [_vp, _vp, _sz, _vp, _sz, _i, C.POINTER(FlowParams), _vp, _sz, _vp]),
    "cart_flow_debug_level": (_i, [_vp, _i, _i, _vp, _sz]),
    "cart_resize_linear": (_i, [_i, _vp, _sz, _i, _i, _i, _vp, _sz, _i, _i, _vp]),
    "cart_copy_narrow": (_i, [_vp, _vp, _vp, _sz, _i, _vp]),
    "cart_find_plane_params": (_i, [C.POINTER(C.c_int32), C.POINTER(PlaneParams)]),
    "cart_find_peaks": (_i, [C.POINTER(C.c_int32), _i] + [C.POINTER(C.c_int)] * 4),
    "cart_debug_read": (_i, [_vp, _i, _i, _vp, _sz]),
    "cart_debug_uniq_table": (_i, [_vp, _i, C.POINTER(C.c_uint16)]),
    "cart_debug_ccl_scratch_nonzero": (_i, [_vp, C.POINTER(C.c_size_t)]),
    "cart_debug_slab_layout": (_i, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "cart_engine_set_timing": (_i, [_vp, _i]),
    "cart_engine_collect_timing": (_i, [_vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), _i, C.POINTER(_i)]),
    "cart_engine_version": (C.c_char_p, []),
}

_lib = None


def load():
    """Loads libcart_engine.so once; raises (loudly) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP engine is not built (run `make -C cart-slam_amd` or "
                "__graft_entry__.build()). There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib
