"""cartslam -- Python plumbing around the MI355X dense-stereo engine (C ABI: include/cart_engine.h).

Only device-memory/stream plumbing, the synthetic scene generator and the frame-sharded batch driver
live here; all arithmetic is in the HIP library (cart-slam_amd/csrc).  Nothing here imports oracle/.
"""
from . import _lib, synth  # noqa: F401
from ._lib import DenseEgoParams, DenseEgoResult, ModelTrackParams, ModelTrackResult, EgoCamera, FusionParams, EgoParams, EngineParams, Keypoint, LocalBAParams, LocalBAResult, Match, MatchParams, MotionParams, ObjectParams, PlaceCandidate, PlaceParams, PlaneMapCell, PlaneMapParams, PlaneParams, PoseGraphParams, PoseGraphResult, SuperpixelParams, Voxel, VoxelMapParams, MeshVertex, MeshQuad  # noqa: F401
from .engine import DENSE_EGO_RESULT_DTYPE, MODEL_TRACK_RESULT_DTYPE, ModelTrack, model_track_params, EGO_HYPOTHESIS_DTYPE, EGO_RESULT_DTYPE, INVALID, LOCAL_BA_RESULT_DTYPE, MATCH_DTYPE, OBJECT_DTYPE, PLACE_CANDIDATE_DTYPE, PLANE_MAP_CELL_DTYPE, POSE_GRAPH_RESULT_DTYPE, TRACK_DTYPE, VOXEL_DTYPE, MESH_VERTEX_DTYPE, MESH_QUAD_DTYPE, write_ply, MotionSegmentation, DenseEgo, DevicePlaneSchedule, DisparityFusion, EgoMotion, Engine, EngineError, LocalBA, ObjectTracker, ObjectTracks, OrbFeatures, OrbMatcher, PlaceDB, PlaneFit, PlaneMap, PlaneStore, PoseGraph, Superpixels, VoxelMap, find_peaks, dense_ego_params, find_plane_params, fusion_params, local_ba_params, motion_params, motion_segment, object_params, orb_levels, place_params, plane_cluster, pose_graph_params, plane_map_params, voxel_map_params  # noqa: F401
