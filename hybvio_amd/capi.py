"""ctypes binding of include/hybvio_hip.h (libhybvio_hip.so).

Python is only the test / bench harness language here: the product is the C-ABI library and the
C++ adapters under hybvio_amd/host/. There is no CPU fallback: if the library cannot be built or
loaded, or no HIP device is present, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

# The torch wheel bundles its own libamdhip64/libhsa-runtime64. A process must initialise exactly
# ONE HIP/HSA runtime, so when torch is installed it is imported BEFORE libhybvio_hip.so is loaded:
# the dynamic linker then resolves our NEEDED libamdhip64.so.7 to the copy torch already mapped.
# (A C++ host such as the reference `main` has no torch and simply uses /opt/rocm.)
try:
    import torch  # noqa: F401
except ImportError:  # pragma: no cover
    torch = None

from . import build as _build

u8p = C.POINTER(C.c_uint8)
i16p = C.POINTER(C.c_int16)
i32p = C.POINTER(C.c_int32)
f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)

HV_MAX_LEVELS = 6
(K_PYR_L0, K_PYR_LN, K_KLT, K_EKF_PREDICT, K_EKF_UPDATE, K_EKF_AUGMENT, K_GFTT, K_INGEST, K_VU_PREPARE, K_ROT_RANSAC, K_EKF_GATE, K_VU_TRI,
 K_SUBPIX, K_RANSAC5, K_STEREO_GATE, K_DETECT_TAIL, K_TRACK_TABLE, K_RANSAC3, K_EKF_CONTROL, K_TRAIL_INDEX) = range(20)
RANSAC5_MAX_ITERS = 75
RANSAC3_MAX_ITERS = 500
UPRIGHT2P_MAX_ITERS = 500
# RansacResult::Type as reported by hv_ransac3_lk_batch_dev
R3_TYPE_SKIPPED, R3_TYPE_R3 = 0, 2
# RansacResult::Type as reported by hv_upright2p_lk_batch_dev
U2_TYPE_SKIPPED, U2_TYPE_UPRIGHT_2P = 0, 4
# RansacResult::Type as reported by hv_hybrid_ransac_lk_batch_dev
R5_TYPE_SKIPPED, R5_TYPE_R2, R5_TYPE_R5 = 0, 1, 3
SUBPIX_MAX_WIN = 16

# tracker::Feature::Status (src/tracker/track.hpp:9-21)
ST_TRACKED, ST_NEW, ST_FAILED_FLOW, ST_RANSAC_OUTLIER, ST_FLOW_OUT_OF_RANGE = 0, 1, 2, 3, 4
ST_OUT_OF_RANGE, ST_FAILED_EPIPOLAR_CHECK, ST_CULLED, ST_BLACKLISTED = 5, 6, 7, 8
DETECTION_FILTER_MAX_POINTS = 1024
TRACKS_MAX_TRACKS = 1024
TRAIL_MAX_POSES, TRAIL_MAX_VISITS = 64, 64
FLOW_PREDICT_LEFT, FLOW_PREDICT_RIGHT, FLOW_PREDICT_STEREO = 0, 1, 2            # OpticalFlowPredictor::Type
TRACK_SAMPLING_GAP, TRACK_SAMPLING_ALL, TRACK_SAMPLING_RANDOM = 0, 1, 2
DETECT_TAIL_MAX_KEYPOINTS, DETECT_TAIL_MAX_CORNERS, DETECT_TAIL_MAX_PREV, DETECT_TAIL_MAX_TRACKS = 16384, 32768, 4096, 4096


class Params(C.Structure):
    _fields_ = [("device", C.c_int), ("width", C.c_int), ("height", C.c_int), ("levels", C.c_int),
                ("win", C.c_int), ("max_iter", C.c_int), ("eps", C.c_double), ("min_eig", C.c_double),
                ("max_tracks", C.c_int), ("pool_size", C.c_int), ("max_pairs", C.c_int)]


class EkfParams(C.Structure):
    _fields_ = [("cameraTrailLength", C.c_int), ("hybridMapSize", C.c_int)] + [
        (k, C.c_double) for k in (
            "noiseScale", "gravity", "augmentR", "initZuptR", "rotationZuptR",
            "noiseInitialPos", "noiseInitialOri", "noiseInitialVel", "noiseInitialPosTrail", "noiseInitialOriTrail",
            "noiseInitialBGA", "noiseInitialBAA", "noiseInitialBAT", "noiseInitialSFT",
            "noiseProcessAcc", "noiseProcessGyro", "noiseProcessBAA", "noiseProcessBGA",
            "noiseProcessBAARev", "noiseProcessBGARev")]


class GfttParams(C.Structure):
    _fields_ = [("gfttBlockSize", C.c_int), ("gfttMinDistance", C.c_double), ("gfttMinResponse", C.c_float),
                ("maxTracks", C.c_int)]


class FastParams(C.Structure):
    _fields_ = [("threshold", C.c_int), ("maxTracks", C.c_int)]


class GfttLegacyParams(C.Structure):
    _fields_ = [("gfttBlockSize", C.c_int), ("gfttQualityLevel", C.c_double), ("gfttMinDistance", C.c_double), ("maxTracks", C.c_int)]


class StereoBmParams(C.Structure):
    _fields_ = [("numDisparities", C.c_int), ("blockSize", C.c_int), ("preFilterCap", C.c_int), ("textureThreshold", C.c_int),
                ("uniquenessRatio", C.c_int), ("speckleWindowSize", C.c_int), ("speckleRange", C.c_int)]


class SubpixParams(C.Structure):
    _fields_ = [("subPixWindowSize", C.c_int), ("subPixMaxIter", C.c_int), ("subPixEpsilon", C.c_double)]


class Ransac5Params(C.Structure):
    _fields_ = [("ransac5Prob", C.c_double), ("ransac5Threshold", C.c_double), ("ransacMaxIters", C.c_int),
                ("ransac2InliersToSkipRansac5", C.c_double), ("ransacMinInlierFraction", C.c_double),
                ("ransac2InliersOverRansac5Needed", C.c_double)]


class Ransac3Params(C.Structure):
    _fields_ = [("ransac3ErrorThresh", C.c_double), ("ransac3FailureProbability", C.c_double), ("ransac3MaxIterations", C.c_int),
                ("ransac3MinIterations", C.c_int), ("ransac3UseMle", C.c_int), ("ransacMinInlierFraction", C.c_double)]


class Upright2pParams(C.Structure):
    _fields_ = [("ransacStereoUpright2pErrorThresh", C.c_double), ("ransacStereoUpright2pFailureProbability", C.c_double),
                ("ransacStereoUpright2pMaxIterations", C.c_int), ("ransacStereoUpright2pMinIterations", C.c_int),
                ("ransacStereoUpright2pUseMle", C.c_int), ("ransacMinInlierFraction", C.c_double)]


class StereoGateParams(C.Structure):
    _fields_ = [("maxStereoEpipolarDistance", C.c_float), ("partOfImageToDetectFeatures", C.c_double), ("fisheyeCamera", C.c_int),
                ("independentStereoOpticalFlow", C.c_int), ("cam0ToCam1", C.c_double * 16)]


class TrackTableParams(C.Structure):
    _fields_ = [("maxTracks", C.c_int), ("maxTrackLength", C.c_int), ("relativeMaskRadius", C.c_double),
                ("visualStationarityMovementThreshold", C.c_double), ("visualStationarityScoreThreshold", C.c_double)]


class TrackTable(C.Structure):
    """hv_track_table: device pointers owned by the caller (second_xy None = mono)."""
    _fields_ = [(k, C.c_void_p) for k in ("n_tracks", "ids", "xy", "second_xy", "status", "blacklist", "kf_xy", "kf_valid",
                                          "frame_num", "mask_steps", "mask_radius", "frame_flags")]


class TrailIndexParams(C.Structure):
    _fields_ = [(k, C.c_int) for k in (
        "cameraTrailLength", "cameraTrailHanoiLength", "cameraTrailStridedLength", "cameraTrailStridedStride", "cameraTrailFixedScheme",
        "trackSampling", "trackMinFrames", "scoreVisualUpdateTracks", "blacklistTracks", "maxVisualUpdates",
        "maxSuccessfulVisualUpdates", "estimateImuCameraTimeShift", "useStereo", "maxTracks", "hybridMapSize",
        "useIndependentStereoTriangulation", "fullPointCloud")]


class TrailIndexTable(C.Structure):
    """hv_trail_index: device pointers owned by the caller."""
    _fields_ = [(k, C.c_void_p) for k in (
        "n_keyframes", "frame_counter", "kf_row", "frame_number", "timestamp", "col_id", "col_len", "image_point", "norm_point",
        "norm_velocity", "used", "n_blacklist", "blacklist_ids", "n_order", "n_skipped", "skipped_pos", "skipped_id", "cand_pos",
        "cand_col")]


class FlowPredictParams(C.Structure):
    """hv_flow_predict_params; cameraToImu / secondCameraToImu are the inverses of the two imuToCamera matrices."""
    _fields_ = [("predictOpticalFlowMinTriangulationDistance", C.c_double), ("minBaselinePoses", C.c_int),
                ("imuToCamera", C.c_double * 16), ("secondImuToCamera", C.c_double * 16),
                ("cameraToImu", C.c_double * 16), ("secondCameraToImu", C.c_double * 16)]


class EkfControlParams(C.Structure):
    _fields_ = [("useDecayingZeroVelocityUpdate", C.c_int), ("usePseudoVelocity", C.c_int), ("pseudoVelocityLimit", C.c_double),
                ("pseudoVelocityTarget", C.c_double), ("pseudoVelocityR", C.c_double), ("useVisualStationarity", C.c_int),
                ("visualStationarityFrameCountThreshold", C.c_int), ("visualZuptR", C.c_double)]


class EkfControlTable(C.Structure):
    """hv_ekf_control: device pointers owned by the caller."""
    _fields_ = [(k, C.c_void_p) for k in ("zupt_time", "init_zupt_time", "was_stationary", "frames_since_keyframe")]


class SessionParams(C.Structure):
    _fields_ = [("targetFps", C.c_double), ("visualUpdateForEveryNFrame", C.c_int), ("goodFramesTimeWindowSeconds", C.c_double),
                ("goodFramesToTracking", C.c_double), ("goodFramesToTrackingFailed", C.c_double), ("resetUntilInitSucceeds", C.c_int),
                ("resetOnFailedTracking", C.c_int), ("resetAfterTrackingFailsToInitialize", C.c_double),
                ("freezeOnFailedTracking", C.c_int)]


class SessionState(C.Structure):
    """hv_session: device pointers owned by the caller."""
    _fields_ = [(k, C.c_void_p) for k in ("good_ring", "ring_head", "ring_entries", "tracking_status", "control_status",
                                          "last_reset_time", "first_sample", "first_sample_t", "prev_sample_t", "time",
                                          "initialized_orientation")]


class OutputParams(C.Structure):
    _fields_ = [("imuToCamera", C.c_double * 16), ("imuToOutput", C.c_double * 16), ("maxVisualUpdates", C.c_int),
                ("maxSuccessfulVisualUpdates", C.c_int), ("cameraTrailLength", C.c_int), ("maxTracks", C.c_int), ("useStereo", C.c_int)]


class OutputFrame(C.Structure):
    """hv_output_frame: what the frame's other entries wrote (device pointers; the last five may be None)."""
    _fields_ = [(k, C.c_void_p) for k in ("cand_id_dev", "n_candidates_dev", "status_dev", "gate_status_dev", "pf_dev",
                                          "tracking_status_dev", "frozen_dev", "stationary_dev", "slam_to_odometry_dev",
                                          "odometry_to_slam_dev", "ready_dev")]


class OutputTable(C.Structure):
    """hv_output: device pointers owned by the caller."""
    _fields_ = [(k, C.c_void_p) for k in ("t", "tracking_status", "stationary_visual", "inertial_mean", "inertial_cov_diag",
                                          "position_cov", "velocity_cov", "n_trail", "trail_time", "trail_pose", "api_pose",
                                          "api_trail_pose", "n_points", "point_id", "point_status", "point_first_pixel", "point_xyz")]


class FullCloudFrame(C.Structure):
    """hv_full_cloud_frame: what select was given and the visit loop wrote (device pointers; full_update_dev, stationary_dev,
    odometry_to_slam_dev and ready_dev may be None)."""
    _fields_ = [(k, C.c_void_p) for k in ("draws_dev", "full_update_dev", "cand_id_dev", "n_candidates_dev", "status_dev",
                                          "gate_status_dev", "pf_dev", "stationary_dev", "odometry_to_slam_dev", "ready_dev")]


class FullCloudTable(C.Structure):
    """hv_full_cloud: device pointers owned by the caller (n_attempts and good_frame may be None)."""
    _fields_ = [(k, C.c_void_p) for k in ("n_points", "point_id", "point_status", "point_first_pixel", "point_xyz", "n_tail", "tail_id",
                                          "tail_status", "tail_col", "tail_pose_mask", "n_attempts", "good_frame")]


class RngState(C.Structure):
    """hv_rng: device pointers owned by the caller."""
    _fields_ = [("mt", C.c_void_p), ("pos", C.c_void_p)]


class IntensityParams(C.Structure):
    _fields_ = [("matchSuccessiveIntensities", C.c_double), ("matchStereoIntensities", C.c_int)]


class IntensityState(C.Structure):
    """hv_intensity_state: device pointers owned by the caller."""
    _fields_ = [(k, C.c_void_p) for k in ("prev_sum", "prev_sqsum", "has_prev", "hist")]


class IntensityRecord(C.Structure):
    """hv_intensity_record (index 0 = left, 1 = right)."""
    _fields_ = [(k, C.c_uint64 * 2) for k in ("in_sum", "in_sqsum", "out_sum", "out_sqsum")] + [
        (k, C.c_double * 2) for k in ("k", "mean0", "mean")] + [("flags", C.c_int32), ("reserved", C.c_int32)]


class HvError(RuntimeError):
    pass


_LIB = None

# name -> (restype, argtypes); also the list of symbols tests check against the header.
PROTOTYPES = {
    "hv_default_params": (None, [C.POINTER(Params)]),
    "hv_abi_version": (C.c_int, []),
    "hv_status_string": (C.c_char_p, [C.c_int]),
    "hv_debug_set_knob": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "hv_debug_get_knob": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    "hv_ekf_frame_error": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "hv_create": (C.c_int, [C.POINTER(Params), C.POINTER(C.c_void_p)]),
    "hv_destroy": (None, [C.c_void_p]),
    "hv_last_error": (C.c_char_p, [C.c_void_p]),
    "hv_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hv_synchronize": (C.c_int, [C.c_void_p]),
    "hv_get_stream": (C.c_void_p, [C.c_void_p]),
    "hv_lanes_create": (C.c_int, [C.POINTER(Params), C.c_int, C.POINTER(C.c_void_p)]),
    "hv_lanes_count": (C.c_int, [C.c_void_p]),
    "hv_lanes_ctx": (C.c_void_p, [C.c_void_p, C.c_int]),
    "hv_lanes_destroy": (None, [C.c_void_p]),
    "hv_pyramid_acquire": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "hv_pyramid_release": (C.c_int, [C.c_void_p, C.c_int]),
    "hv_pyramid_level_size": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hv_pyramid_build": (C.c_int, [C.c_void_p, C.c_int, u8p, C.c_int]),
    "hv_ingest_set_undistort_map": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hv_ingest_build": (C.c_int, [C.c_void_p, C.c_int, u8p, C.c_int, C.c_int, C.c_int]),
    "hv_ingest_build_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int]),
    "hv_pyramid_build_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int]),
    "hv_pyramid_download": (C.c_int, [C.c_void_p, C.c_int, C.c_int, u8p, i16p]),
    "hv_klt_track": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, f32p, f32p, u8p, f32p, C.c_int, C.c_int]),
    "hv_optical_flow_compute": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, f32p, f32p, i32p, C.c_int, C.c_int]),
    "hv_klt_track_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "hv_klt_track_batch_ragged_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "hv_ekf_default_params": (None, [C.POINTER(EkfParams)]),
    "hv_ekf_create": (C.c_int, [C.c_void_p, C.POINTER(EkfParams), C.c_int, C.POINTER(C.c_void_p)]),
    "hv_ekf_destroy": (None, [C.c_void_p]),
    "hv_ekf_state_dim": (C.c_int, [C.c_void_p]),
    "hv_ekf_batch": (C.c_int, [C.c_void_p]),
    "hv_ekf_set_state": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p]),
    "hv_ekf_get_state": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p]),
    "hv_ekf_get_means": (C.c_int, [C.c_void_p, f64p]),
    "hv_ekf_set_process_noise": (C.c_int, [C.c_void_p, C.c_int, f64p]),
    "hv_ekf_get_process_noise": (C.c_int, [C.c_void_p, C.c_int, f64p]),
    "hv_ekf_get_dydx": (C.c_int, [C.c_void_p, C.c_int, f64p]),
    "hv_ekf_device_pointers": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "hv_ekf_predict": (C.c_int, [C.c_void_p, f64p, f64p, f64p]),
    "hv_ekf_predict_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hv_ekf_predict_n_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hv_ekf_predict_n": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p, f64p]),
    "hv_ekf_update": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f64p, f64p, f64p, u8p, C.c_int]),
    "hv_ekf_visual_gate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f64p, f64p, C.c_double, f64p, i32p]),
    "hv_ekf_visual_update": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f64p, f64p, C.c_double, u8p]),
    "hv_camera_model_init": (C.c_int, [C.c_void_p]),
    "hv_rot_ransac": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_float] + [C.c_void_p] * 4),
    "hv_rot_ransac_lk_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3 + [C.c_float] + [C.c_void_p] * 3),
    "hv_rot_ransac_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_float] + [C.c_void_p] * 3),
    "hv_vu_default_params": (None, [C.c_void_p]),
    "hv_ekf_visual_prepare_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 10),
    "hv_ekf_visual_track_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_double, C.c_double] + [C.c_void_p] * 4),
    "hv_ekf_visual_track_hybrid_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_double, C.c_double] + [C.c_void_p] * 4),
    "hv_ekf_visual_track_limited_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_double, C.c_double] + [C.c_void_p] * 5 + [C.c_int]),
    "hv_ekf_visual_track": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_double, C.c_double] + [C.c_void_p] * 4),
    "hv_ekf_visual_frame_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_double, C.c_double] + [C.c_void_p] * 5 + [C.c_int]),
    "hv_ekf_visual_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_double, C.c_double] + [C.c_void_p] * 5 + [C.c_int]),
    "hv_ekf_visual_frame_ragged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_double, C.c_double] + [C.c_void_p] * 5 + [C.c_int]),
    "hv_ekf_visual_frame_ragged_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_double, C.c_double] + [C.c_void_p] * 5 + [C.c_int]),
    "hv_ekf_visual_frame_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_double, C.c_double] + [C.c_void_p] * 5 + [C.c_int, C.c_int]),
    "hv_ekf_augment_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hv_ekf_symmetrize_augment_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    # ABI 4: host-pointer forms of the r04 frame entries + map points on the resident state
    "hv_ekf_symmetrize_augment": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hv_ekf_visual_frame_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_double, C.c_double] + [C.c_void_p] * 5 + [C.c_int, C.c_int]),
    "hv_ekf_visual_track_hybrid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_double, C.c_double] + [C.c_void_p] * 4),
    "hv_ekf_insert_map_point": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "hv_ekf_get_map_point": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "hv_ekf_visual_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int,
                                    C.c_void_p, C.c_void_p]),
    "hv_ekf_augment": (C.c_int, [C.c_void_p, i32p, u8p]),
    "hv_ekf_undo_augment": (C.c_int, [C.c_void_p, u8p]),
    "hv_ekf_symmetrize": (C.c_int, [C.c_void_p]),
    "hv_ekf_normalize_quaternions": (C.c_int, [C.c_void_p, C.c_int]),
    "hv_ekf_transform": (C.c_int, [C.c_void_p, C.c_int, f64p, f64p, f64p]),
    "hv_gftt_default_params": (None, [C.POINTER(GfttParams)]),
    "hv_gftt_block_size": (C.c_int, [C.POINTER(GfttParams)]),
    "hv_gftt_keypoint_count": (C.c_int, [C.c_void_p, C.POINTER(GfttParams)]),
    "hv_gftt_detect": (C.c_int, [C.c_void_p, C.POINTER(GfttParams), C.c_int, f32p, C.c_int, C.c_int, f32p, C.c_int,
                                 C.POINTER(C.c_int)]),
    "hv_gftt_keypoints_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(GfttParams), C.c_int, C.c_void_p, C.c_void_p]),
    "hv_apply_min_distance_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_int, C.c_void_p]),
    "hv_gftt_corners_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(GfttParams), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hv_gftt_detect_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(GfttParams), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hv_apply_min_distance": (None, [f32p, C.POINTER(C.c_int), f32p, C.c_int, C.c_int, C.c_int]),
    "hv_fast_default_params": (None, [C.POINTER(FastParams)]),
    "hv_fast_tile_size": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hv_fast_keypoint_bound": (C.c_int, [C.c_void_p]),
    "hv_fast_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "hv_fast_keypoints_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(FastParams), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p]),
    "hv_fast_detect_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(FastParams), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hv_fast_detect": (C.c_int, [C.c_void_p, C.POINTER(FastParams), C.c_int, f32p, C.c_int, C.c_int, f32p, C.c_int,
                                 C.POINTER(C.c_int)]),
    "hv_gftt_legacy_default_params": (None, [C.POINTER(GfttLegacyParams)]),
    "hv_gftt_legacy_tile_size": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hv_gftt_legacy_min_distance": (C.c_double, [C.c_void_p, C.POINTER(GfttLegacyParams)]),
    "hv_gftt_legacy_keypoint_bound": (C.c_int, [C.c_void_p]),
    "hv_gftt_legacy_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "hv_gftt_legacy_keypoints_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(GfttLegacyParams), C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hv_gftt_legacy_detect_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(GfttLegacyParams), C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                  C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]),
    "hv_gftt_legacy_detect": (C.c_int, [C.c_void_p, C.POINTER(GfttLegacyParams), C.c_int, f32p, C.c_int, C.c_int, f32p, C.c_int,
                                        C.POINTER(C.c_int)]),
    "hv_stereo_num_disparities": (C.c_int, [C.c_int]),
    "hv_stereo_bm_default_params": (None, [C.POINTER(StereoBmParams), C.c_int]),
    "hv_stereo_work_bytes": (C.c_size_t, [C.c_void_p, C.POINTER(StereoBmParams), C.c_int]),
    "hv_filter_speckles_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hv_stereo_cloud_bound": (C.c_int, [C.c_void_p, C.c_int]),
    "hv_stereo_disparity_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(StereoBmParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_longlong, C.c_void_p]),
    "hv_filter_speckles_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_int,
                                               C.c_int, C.c_void_p]),
    "hv_stereo_track_depth_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong,
                                                  C.POINTER(C.c_double), C.c_void_p]),
    "hv_stereo_point_cloud_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.POINTER(C.c_double), C.c_int,
                                                  C.c_int, C.c_void_p, C.c_void_p]),
    "hv_stereo_disparity": (C.c_int, [C.c_void_p, C.POINTER(StereoBmParams), C.c_int, C.c_int, C.c_void_p, C.c_longlong]),
    "hv_stereo_track_depth": (C.c_int, [C.c_void_p, C.c_int, f32p, C.c_void_p, C.c_longlong, C.POINTER(C.c_double), f32p]),
    "hv_stereo_point_cloud": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.POINTER(C.c_double), C.c_int, f32p, C.c_int,
                                        C.POINTER(C.c_int)]),
    "hv_subpix_default_params": (None, [C.POINTER(SubpixParams)]),
    "hv_corner_subpix": (C.c_int, [C.c_void_p, C.POINTER(SubpixParams), C.c_int, C.c_int, f32p, i32p]),
    "hv_corner_subpix_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(SubpixParams), C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "hv_ransac5_default_params": (None, [C.POINTER(Ransac5Params)]),
    "hv_ransac5": (C.c_int, [C.c_void_p, C.POINTER(Ransac5Params), C.c_int] + [C.c_void_p] * 7),
    "hv_ransac5_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(Ransac5Params), C.c_int, C.c_int] + [C.c_void_p] * 8),
    "hv_hybrid_ransac_lk_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(Ransac5Params), C.c_int, C.c_int] + [C.c_void_p] * 12),
    "hv_ransac3_default_params": (None, [C.POINTER(Ransac3Params)]),
    "hv_ransac3": (C.c_int, [C.c_void_p, C.POINTER(Ransac3Params), C.c_int] + [C.c_void_p] * 10),
    "hv_ransac3_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(Ransac3Params), C.c_int, C.c_int] + [C.c_void_p] * 11),
    "hv_ransac3_lk_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(Ransac3Params), C.c_int, C.c_int] + [C.c_void_p] * 14),
    "hv_stereo_gate_default_params": (None, [C.POINTER(StereoGateParams)]),
    "hv_flow_status_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4),
    "hv_track_gate": (C.c_int, [C.c_void_p, C.POINTER(StereoGateParams), C.c_int] + [C.c_void_p] * 7),
    "hv_track_gate_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(StereoGateParams), C.c_int, C.c_int] + [C.c_void_p] * 9),
    "hv_detection_filter": (C.c_int, [C.c_void_p, C.POINTER(StereoGateParams), C.c_int] + [C.c_void_p] * 9),
    "hv_detection_filter_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(StereoGateParams), C.c_int, C.c_int] + [C.c_void_p] * 10),
    "hv_track_table_default_params": (None, [C.POINTER(TrackTableParams)]),
    "hv_tracks_init_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(TrackTableParams), C.c_int, C.POINTER(TrackTable)]),
    "hv_tracks_update_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(TrackTableParams), C.c_int, C.POINTER(TrackTable)] + [C.c_void_p] * 9),
    "hv_tracks_append_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(TrackTableParams), C.c_int, C.POINTER(TrackTable), C.c_int]
                                   + [C.c_void_p] * 4),
    "hv_tracks_delete_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(TrackTableParams), C.c_int, C.POINTER(TrackTable), C.c_int]
                                   + [C.c_void_p] * 2),
    "hv_ekf_block_update_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_void_p]),
    "hv_ekf_pseudo_velocity_dev": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "hv_ekf_undo_augment_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hv_ekf_control_default_params": (None, [C.POINTER(EkfControlParams)]),
    "hv_ekf_control_init_dev": (C.c_int, [C.c_void_p, C.POINTER(EkfControlTable)]),
    "hv_ekf_imu_control_dev": (C.c_int, [C.c_void_p, C.POINTER(EkfControlParams), C.POINTER(EkfControlTable), C.c_void_p, C.c_void_p]),
    "hv_ekf_frame_control_dev": (C.c_int, [C.c_void_p, C.POINTER(EkfControlParams), C.POINTER(EkfControlTable)] + [C.c_void_p] * 7),
    "hv_trail_index_default_params": (None, [C.POINTER(TrailIndexParams)]),
    "hv_trail_init_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(TrailIndexParams), C.c_int, C.POINTER(TrailIndexTable)]),
    "hv_trail_select_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(TrailIndexParams), C.c_int, C.POINTER(TrailIndexTable),
                                            C.POINTER(TrackTable), C.c_void_p, C.c_void_p] + [C.c_void_p] * 13),
    "hv_trail_finish_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(TrailIndexParams), C.c_int, C.POINTER(TrailIndexTable)]
                                  + [C.c_void_p] * 11),
    "hv_upright2p_default_params": (None, [C.POINTER(Upright2pParams)]),
    "hv_upright2p": (C.c_int, [C.c_void_p, C.POINTER(Upright2pParams), C.c_int] + [C.c_void_p] * 11),
    "hv_upright2p_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(Upright2pParams), C.c_int, C.c_int] + [C.c_void_p] * 12),
    "hv_upright2p_lk_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(Upright2pParams), C.POINTER(FlowPredictParams), C.c_int] + [C.c_void_p] * 14),
    "hv_flow_predict_default_params": (None, [C.POINTER(FlowPredictParams)]),
    "hv_flow_predict_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(FlowPredictParams), C.c_int, C.POINTER(TrailIndexParams),
                                            C.POINTER(TrailIndexTable), C.POINTER(TrackTable)] + [C.c_void_p] * 5 + [C.c_int]),
    "hv_session_default_params": (None, [C.POINTER(SessionParams)]),
    "hv_session_init_dev": (C.c_int, [C.c_void_p, C.POINTER(SessionParams), C.POINTER(SessionState)]),
    "hv_session_imu_dev": (C.c_int, [C.c_void_p, C.POINTER(SessionState), C.c_int] + [C.c_void_p] * 5),
    "hv_session_status_dev": (C.c_int, [C.c_void_p, C.POINTER(SessionParams), C.POINTER(SessionState)] + [C.c_void_p] * 5),
    "hv_session_reset_dev": (C.c_int, [C.c_void_p, C.POINTER(SessionParams), C.POINTER(SessionState), C.POINTER(EkfControlTable),
                                       C.POINTER(TrackTableParams), C.POINTER(TrackTable), C.POINTER(TrailIndexParams),
                                       C.POINTER(TrailIndexTable), C.c_void_p]),
    "hv_output_default_params": (None, [C.POINTER(OutputParams)]),
    "hv_output_dev": (C.c_int, [C.c_void_p, C.POINTER(OutputParams), C.POINTER(SessionState), C.POINTER(TrailIndexTable),
                                C.POINTER(OutputFrame), C.POINTER(OutputTable)]),
    "hv_full_point_cloud_dev": (C.c_int, [C.c_void_p, C.POINTER(TrailIndexParams), C.c_void_p, C.POINTER(TrailIndexTable),
                                          C.POINTER(TrackTable), C.POINTER(FullCloudFrame), C.POINTER(FullCloudTable)]),
    "hv_rng_seed_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RngState), C.c_uint32, C.c_void_p, C.c_void_p]),
    "hv_rng_draw_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RngState), C.c_int, C.c_void_p]),
    "hv_rng_advance_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RngState), C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "hv_intensity_default_params": (None, [C.POINTER(IntensityParams)]),
    "hv_intensity_init_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(IntensityState)]),
    "hv_match_intensities_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(IntensityParams), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                 C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.POINTER(IntensityState),
                                                 C.c_void_p, C.c_void_p]),
    "hv_match_intensities": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double]),
    "hv_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "hv_profile_reset": (C.c_int, [C.c_void_p]),
    "hv_profile_read": (C.c_int, [C.c_void_p, C.c_int, f64p, C.POINTER(C.c_longlong)]),
}


def lib():
    """Load (building if needed) libhybvio_hip.so. Raises if it cannot be produced."""
    global _LIB
    if _LIB is None:
        path = _build.build_hip()
        # HV_LIB_OVERRIDE (developer A/B runs only): another build of the same library, e.g. the previous commit's, in the same process setup
        path = os.environ.get("HV_LIB_OVERRIDE", path)
        if not os.path.exists(path):
            raise HvError(f"{path} missing: the HIP extension is required, there is no fallback")
        L = C.CDLL(path)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


class Context:
    """One hv_ctx: a HIP stream, a pool of pyramid slots and the tracker parameters."""

    def __init__(self, width=752, height=480, levels=4, win=31, max_iter=20, eps=0.03, min_eig=1e-3,
                 max_tracks=200, pool_size=16, max_pairs=1, device=0, _adopt=None):
        L = lib()
        p = Params()
        L.hv_default_params(C.byref(p))
        p.device, p.width, p.height, p.levels, p.win = device, width, height, levels, win
        p.max_iter, p.eps, p.min_eig, p.max_tracks = max_iter, eps, min_eig, max_tracks
        p.pool_size, p.max_pairs = pool_size, max_pairs
        self.params = p
        self._owned = _adopt is None
        if _adopt is not None:                       # a lane of a Lanes set: the set owns the hv_ctx
            self._h = C.c_void_p(_adopt)
        else:
            self._h = C.c_void_p()
            rc = L.hv_create(C.byref(p), C.byref(self._h))
            if rc != 0:
                self._h = None
                raise HvError(f"hv_create: {L.hv_status_string(rc).decode()}")
        self.levels = 0
        self.level_sizes = []
        w, h = C.c_int(), C.c_int()
        while self.levels < levels and L.hv_pyramid_level_size(self._h, self.levels, C.byref(w), C.byref(h)) == 0:
            self.level_sizes.append((w.value, h.value))
            self.levels += 1

    def close(self):
        if getattr(self, "_h", None):
            for child in list(getattr(self, "_children", [])):   # hv_ekf objects must die before their hv_ctx
                child.close()
            if self._owned:
                lib().hv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:                             # interpreter shutdown: module globals may be gone already
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc, what):
        if rc != 0:
            L = lib()
            msg = L.hv_status_string(rc).decode()
            if rc == -4:
                msg += ": " + L.hv_last_error(self._h).decode()
            raise HvError(f"{what}: {msg}")

    # -- plumbing --
    def set_knob(self, name: str, value: int):
        """Force a kernel variant (tests / measurements; include/hybvio_hip.h hv_debug_set_knob)."""
        self._chk(lib().hv_debug_set_knob(self._h, name.encode(), int(value)), f"hv_debug_set_knob({name})")

    def get_knob(self, name: str) -> int:
        v = C.c_int()
        self._chk(lib().hv_debug_get_knob(self._h, name.encode(), C.byref(v)), f"hv_debug_get_knob({name})")
        return v.value

    def set_stream(self, stream_ptr: int):
        self._chk(lib().hv_set_stream(self._h, C.c_void_p(stream_ptr)), "hv_set_stream")

    def get_stream(self) -> int:
        """The hipStream_t the context issues on (hv_get_stream), as an integer handle."""
        return int(lib().hv_get_stream(self._h) or 0)

    def synchronize(self):
        self._chk(lib().hv_synchronize(self._h), "hv_synchronize")

    # -- pyramid --
    def acquire(self) -> int:
        s = C.c_int()
        self._chk(lib().hv_pyramid_acquire(self._h, C.byref(s)), "hv_pyramid_acquire")
        return s.value

    def release(self, slot: int):
        self._chk(lib().hv_pyramid_release(self._h, slot), "hv_pyramid_release")

    def build(self, slot: int, gray: np.ndarray):
        gray = np.ascontiguousarray(gray, np.uint8)
        assert gray.shape == (self.params.height, self.params.width), gray.shape
        self._chk(lib().hv_pyramid_build(self._h, slot, _p(gray, u8p), gray.strides[0]), "hv_pyramid_build")
        self.synchronize()   # the numpy temporary may die after return

    def build_batch_dev(self, n: int, slots_dev: int, gray_dev: int, image_stride: int, row_stride: int):
        self._chk(lib().hv_pyramid_build_batch_dev(self._h, n, C.c_void_p(slots_dev), C.c_void_p(gray_dev),
                                                   image_stride, row_stride), "hv_pyramid_build_batch_dev")

    # ---- 2-point rotation RANSAC (f4) ----
    def rot_ransac(self, c1, c2, cam1: "CameraModel", cam2: "CameraModel", pairs, threshold_pow2: float):
        """hv_rot_ransac: returns (status [n], R 3x3 f32, bestInlierCount, hypotheses visited)."""
        a, b = np.ascontiguousarray(c1, np.float32).reshape(-1, 2), np.ascontiguousarray(c2, np.float32).reshape(-1, 2)
        pr = np.ascontiguousarray(pairs, np.int32).reshape(100, 2)
        st, R = np.zeros(len(a), np.int32), np.zeros((3, 3), np.float32)
        best, vis = C.c_int(0), C.c_int(0)
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(lib().hv_rot_ransac(self._h, len(a), vp(a), vp(b), C.byref(cam1), C.byref(cam2), vp(pr), float(threshold_pow2),
                                      vp(st), vp(R), C.byref(best), C.byref(vis)), "hv_rot_ransac")
        return st, R, best.value, vis.value

    def rot_ransac_batch_dev(self, n_sets, max_points, n_points_dev, c1_dev, c2_dev, cam1, cam2, pairs_dev, threshold_pow2,
                             status_dev, R_dev, summary_dev):
        p = lambda x: C.c_void_p(x)
        self._chk(lib().hv_rot_ransac_batch_dev(self._h, n_sets, max_points, p(n_points_dev), p(c1_dev), p(c2_dev), C.byref(cam1),
                                                C.byref(cam2), p(pairs_dev), float(threshold_pow2), p(status_dev), p(R_dev),
                                                p(summary_dev)), "hv_rot_ransac_batch_dev")

    def rot_ransac_lk_batch_dev(self, n_sets, max_points, n_points_dev, c1_dev, c2_dev, lk_status_dev, lk_tracked_value, cam1, cam2,
                                draws_dev, threshold_pow2, status_dev, R_dev, summary_dev):
        p = lambda x: C.c_void_p(x)
        self._chk(lib().hv_rot_ransac_lk_batch_dev(self._h, n_sets, max_points, p(n_points_dev), p(c1_dev), p(c2_dev), p(lk_status_dev),
                                                   int(lk_tracked_value), C.byref(cam1), C.byref(cam2), p(draws_dev),
                                                   float(threshold_pow2), p(status_dev), p(R_dev), p(summary_dev)),
                  "hv_rot_ransac_lk_batch_dev")

    # ---- five-point RANSAC and the hybrid RANSAC2 / RANSAC5 filter ----
    def ransac5(self, c1, c2, cam1: "CameraModel", cam2: "CameraModel", params: "Ransac5Params" = None):
        """hv_ransac5 (doRansac5): returns (status [n] 0 / 3, E [9], summary [inliers, best iteration, iterations, valid])."""
        rp = params if params is not None else ransac5_default_params()
        a, b = np.ascontiguousarray(c1, np.float32).reshape(-1, 2), np.ascontiguousarray(c2, np.float32).reshape(-1, 2)
        st, E, sm = np.zeros(len(a), np.int32), np.zeros(9), np.zeros(4, np.int32)
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(lib().hv_ransac5(self._h, C.byref(rp), len(a), vp(a), vp(b), C.byref(cam1), C.byref(cam2), vp(st), vp(E), vp(sm)),
                  "hv_ransac5")
        return st, E, sm

    def ransac5_batch_dev(self, n_sets, max_points, n_points_dev, c1_dev, c2_dev, cam1, cam2, status_dev, E_dev=0, summary_dev=0,
                          params: "Ransac5Params" = None):
        rp = params if params is not None else ransac5_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_ransac5_batch_dev(self._h, C.byref(rp), n_sets, max_points, p(n_points_dev), p(c1_dev), p(c2_dev),
                                             C.byref(cam1), C.byref(cam2), p(status_dev), p(E_dev), p(summary_dev)),
                  "hv_ransac5_batch_dev")

    def hybrid_ransac_lk_batch_dev(self, n_sets, max_points, n_points_dev, c1_dev, c2_dev, track_status_dev, r2_status_dev,
                                   r2_summary_dev, cam1, cam2, result_dev, score_dev, E_dev=0, r5_summary_dev=0,
                                   params: "Ransac5Params" = None):
        rp = params if params is not None else ransac5_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_hybrid_ransac_lk_batch_dev(self._h, C.byref(rp), n_sets, max_points, p(n_points_dev), p(c1_dev), p(c2_dev),
                                                      p(track_status_dev), p(r2_status_dev), p(r2_summary_dev), C.byref(cam1),
                                                      C.byref(cam2), p(result_dev), p(score_dev), p(E_dev), p(r5_summary_dev)),
                  "hv_hybrid_ransac_lk_batch_dev")

    # ---- stereo RANSAC3 (P3P absolute pose) ----
    def ransac3(self, status, prev_left, prev_right, cur_left, cam0: "CameraModel", cam1: "CameraModel", second_to_first, draws,
                params: "Ransac3Params" = None):
        """hv_ransac3 (doRansac3): returns (new status [n], pose [12] = R row-major + position, summary [inliers, best
        iteration, iterations run, correspondences]); draws = 3 * ransac3MaxIterations raw std::mt19937 outputs."""
        rp = params if params is not None else ransac3_default_params()
        a, b, c = (np.ascontiguousarray(x, np.float32).reshape(-1, 2) for x in (prev_left, prev_right, cur_left))
        st = np.ascontiguousarray(status, np.int32).copy()
        T = np.ascontiguousarray(second_to_first, np.float64).reshape(16)
        dr = np.ascontiguousarray(draws, np.uint32).reshape(-1)
        assert len(a) == len(b) == len(c) == len(st) and len(dr) >= 3 * rp.ransac3MaxIterations
        pose, sm = np.zeros(12), np.zeros(4, np.int32)
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(lib().hv_ransac3(self._h, C.byref(rp), len(a), vp(a), vp(b), vp(c), C.byref(cam0), C.byref(cam1), vp(T), vp(dr),
                                   vp(st), vp(pose), vp(sm)), "hv_ransac3")
        return st, pose, sm

    def ransac3_batch_dev(self, n_sets, max_points, n_points_dev, prev_left_dev, prev_right_dev, cur_left_dev, cam0, cam1,
                          second_to_first, draws_dev, status_dev, pose_dev=0, summary_dev=0, params: "Ransac3Params" = None):
        rp = params if params is not None else ransac3_default_params()
        T = np.ascontiguousarray(second_to_first, np.float64).reshape(16)          # (copied by the call: a kernel argument)
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_ransac3_batch_dev(self._h, C.byref(rp), n_sets, max_points, p(n_points_dev), p(prev_left_dev),
                                             p(prev_right_dev), p(cur_left_dev), C.byref(cam0), C.byref(cam1),
                                             T.ctypes.data_as(C.c_void_p), p(draws_dev), p(status_dev), p(pose_dev), p(summary_dev)),
                  "hv_ransac3_batch_dev")

    def ransac3_lk_batch_dev(self, n_sets, max_points, n_points_dev, prev_left_dev, prev_right_dev, cur_left_dev, track_status_dev,
                             r2_summary_dev, cam0, cam1, second_to_first, draws_dev, result_dev, score_dev, pose_dev=0,
                             summary_dev=0, params: "Ransac3Params" = None):
        rp = params if params is not None else ransac3_default_params()
        T = np.ascontiguousarray(second_to_first, np.float64).reshape(16)
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_ransac3_lk_batch_dev(self._h, C.byref(rp), n_sets, max_points, p(n_points_dev), p(prev_left_dev),
                                                p(prev_right_dev), p(cur_left_dev), p(track_status_dev), p(r2_summary_dev),
                                                C.byref(cam0), C.byref(cam1), T.ctypes.data_as(C.c_void_p), p(draws_dev),
                                                p(result_dev), p(score_dev), p(pose_dev), p(summary_dev)),
                  "hv_ransac3_lk_batch_dev")

    # ---- stereo upright 2-point RANSAC (rotation about gravity + translation) ----
    def upright2p(self, status, prev_left, prev_right, cur_left, cam0: "CameraModel", cam1: "CameraModel", second_to_first, poses,
                  draws, params: "Upright2pParams" = None):
        """hv_upright2p (StereoUpright2p::compute): poses = the two camera-to-world 4x4 of the previous and the current frame;
        returns (new status [n], model [12] = R row-major + t, summary [inliers, best iteration, iterations run,
        correspondences]); draws = 2 * ransacStereoUpright2pMaxIterations raw std::mt19937 outputs."""
        rp = params if params is not None else upright2p_default_params()
        a, b, c = (np.ascontiguousarray(x, np.float32).reshape(-1, 2) for x in (prev_left, prev_right, cur_left))
        st = np.ascontiguousarray(status, np.int32).copy()
        T = np.ascontiguousarray(second_to_first, np.float64).reshape(16)
        P = np.ascontiguousarray(poses, np.float64).reshape(32)
        dr = np.ascontiguousarray(draws, np.uint32).reshape(-1)
        assert len(a) == len(b) == len(c) == len(st) and len(dr) >= 2 * rp.ransacStereoUpright2pMaxIterations
        model, sm = np.zeros(12), np.zeros(4, np.int32)
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(lib().hv_upright2p(self._h, C.byref(rp), len(a), vp(a), vp(b), vp(c), C.byref(cam0), C.byref(cam1), vp(T), vp(P), vp(dr),
                                     vp(st), vp(model), vp(sm)), "hv_upright2p")
        return st, model, sm

    def upright2p_batch_dev(self, n_sets, max_points, n_points_dev, prev_left_dev, prev_right_dev, cur_left_dev, cam0, cam1,
                            second_to_first, poses_dev, draws_dev, status_dev, model_dev=0, summary_dev=0,
                            params: "Upright2pParams" = None):
        rp = params if params is not None else upright2p_default_params()
        T = np.ascontiguousarray(second_to_first, np.float64).reshape(16)          # (copied by the call: a kernel argument)
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_upright2p_batch_dev(self._h, C.byref(rp), n_sets, max_points, p(n_points_dev), p(prev_left_dev),
                                               p(prev_right_dev), p(cur_left_dev), C.byref(cam0), C.byref(cam1),
                                               T.ctypes.data_as(C.c_void_p), p(poses_dev), p(draws_dev), p(status_dev), p(model_dev),
                                               p(summary_dev)), "hv_upright2p_batch_dev")

    # ---- stereo track gate: flow status, epipolar check, crop, blacklist and the detection filter ----
    def flow_status_batch_dev(self, n_sets, max_points, n_points_dev, xy_dev, lk_status_dev, status_dev):
        """hv_flow_status_batch_dev: LK uint8 status + level-0 range test -> int32 Feature::Status, on the device."""
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_flow_status_batch_dev(self._h, n_sets, max_points, p(n_points_dev), p(xy_dev), p(lk_status_dev), p(status_dev)),
                  "hv_flow_status_batch_dev")

    def track_gate(self, corners, second_corners, stereo_status, track_status, cam0: "CameraModel", cam1: "CameraModel" = None,
                   blacklist=None, params: "StereoGateParams" = None):
        """hv_track_gate (tracker.cpp:441-478): returns the new int32 track statuses; second_corners None = mono."""
        gp = params if params is not None else stereo_gate_default_params()
        a = np.ascontiguousarray(corners, np.float32).reshape(-1, 2)
        b = None if second_corners is None else np.ascontiguousarray(second_corners, np.float32).reshape(-1, 2)
        ss = None if stereo_status is None else np.ascontiguousarray(stereo_status, np.int32)
        bl = None if blacklist is None else np.ascontiguousarray(blacklist, np.uint8)
        ts = np.array(track_status, np.int32).copy()
        vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        self._chk(lib().hv_track_gate(self._h, C.byref(gp), len(a), vp(a), vp(b), vp(ss), vp(bl), C.byref(cam0),
                                      C.byref(cam1) if cam1 is not None else None, vp(ts)), "hv_track_gate")
        return ts

    def track_gate_batch_dev(self, n_sets, max_points, n_points_dev, corners_dev, second_corners_dev, stereo_status_dev, blacklist_dev,
                             cam0, cam1, track_status_dev, tracked_mask_dev=0, params: "StereoGateParams" = None):
        gp = params if params is not None else stereo_gate_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_track_gate_batch_dev(self._h, C.byref(gp), n_sets, max_points, p(n_points_dev), p(corners_dev),
                                                p(second_corners_dev), p(stereo_status_dev), p(blacklist_dev), C.byref(cam0),
                                                C.byref(cam1) if cam1 is not None else None, p(track_status_dev), p(tracked_mask_dev)),
                  "hv_track_gate_batch_dev")

    def detection_filter(self, corners, second_corners, stereo_status, cam0: "CameraModel", cam1: "CameraModel" = None,
                         params: "StereoGateParams" = None):
        """hv_detection_filter (tracker.cpp:266-311) -> (kept corners [m, 2], kept right corners [m, 2] or None, statuses [n])."""
        gp = params if params is not None else stereo_gate_default_params()
        a = np.ascontiguousarray(corners, np.float32).reshape(-1, 2)
        b = None if second_corners is None else np.ascontiguousarray(second_corners, np.float32).reshape(-1, 2)
        ss = None if stereo_status is None else np.ascontiguousarray(stereo_status, np.int32)
        oa, ob = np.zeros_like(a), None if b is None else np.zeros_like(b)
        st, n = np.zeros(len(a), np.int32), C.c_int(-1)
        vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        self._chk(lib().hv_detection_filter(self._h, C.byref(gp), len(a), vp(a), vp(b), vp(ss), C.byref(cam0),
                                            C.byref(cam1) if cam1 is not None else None, vp(st), vp(oa), vp(ob), C.byref(n)),
                  "hv_detection_filter")
        return oa[:n.value].copy(), None if ob is None else ob[:n.value].copy(), st

    def detection_filter_batch_dev(self, n_sets, max_points, n_points_dev, corners_dev, second_corners_dev, stereo_status_dev, cam0, cam1,
                                   status_dev, out_corners_dev, out_second_dev, n_out_dev, params: "StereoGateParams" = None):
        gp = params if params is not None else stereo_gate_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_detection_filter_batch_dev(self._h, C.byref(gp), n_sets, max_points, p(n_points_dev), p(corners_dev),
                                                      p(second_corners_dev), p(stereo_status_dev), C.byref(cam0),
                                                      C.byref(cam1) if cam1 is not None else None, p(status_dev), p(out_corners_dev),
                                                      p(out_second_dev), p(n_out_dev)),
                  "hv_detection_filter_batch_dev")

    # ---- device track table: updateTracks, culling, keyframes, new-track append and deleteTrack ----
    def tracks_init_batch_dev(self, n_sets, table: "TrackTable", params: "TrackTableParams" = None):
        tp = params if params is not None else track_table_default_params()
        self._chk(lib().hv_tracks_init_batch_dev(self._h, C.byref(tp), n_sets, C.byref(table)), "hv_tracks_init_batch_dev")

    def tracks_update_batch_dev(self, n_sets, table: "TrackTable", corners_dev, second_corners_dev, track_status_dev, score_dev,
                                keyframe_dev, mask_xy_dev, n_mask_dev, src_index_dev=0, max_movement_dev=0,
                                params: "TrackTableParams" = None):
        """hv_tracks_update_batch_dev (tracker.cpp:527-530, 578-670, 766-777): mask, keyframe, culling, write-back and compaction."""
        tp = params if params is not None else track_table_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_tracks_update_batch_dev(self._h, C.byref(tp), n_sets, C.byref(table), p(corners_dev), p(second_corners_dev),
                                                   p(track_status_dev), p(score_dev), p(keyframe_dev), p(mask_xy_dev), p(n_mask_dev),
                                                   p(src_index_dev), p(max_movement_dev)),
                  "hv_tracks_update_batch_dev")

    def tracks_append_batch_dev(self, n_sets, table: "TrackTable", max_new, n_new_dev, new_xy_dev, new_second_dev, n_added_dev=0,
                                params: "TrackTableParams" = None):
        """hv_tracks_append_batch_dev (tracker.cpp:199, 540-546, 672-719): new tracks, IDs, mask tuning, frame_num."""
        tp = params if params is not None else track_table_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_tracks_append_batch_dev(self._h, C.byref(tp), n_sets, C.byref(table), max_new, p(n_new_dev), p(new_xy_dev),
                                                   p(new_second_dev), p(n_added_dev)),
                  "hv_tracks_append_batch_dev")

    def tracks_delete_batch_dev(self, n_sets, table: "TrackTable", max_ids, n_ids_dev, ids_dev, params: "TrackTableParams" = None):
        """hv_tracks_delete_batch_dev (deleteTrack, tracker.cpp:726-738)."""
        tp = params if params is not None else track_table_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_tracks_delete_batch_dev(self._h, C.byref(tp), n_sets, C.byref(table), max_ids, p(n_ids_dev), p(ids_dev)),
                  "hv_tracks_delete_batch_dev")

    # ---- device pose-trail index: keyframes, visual-update track selection, blacklist ----
    def trail_init_batch_dev(self, n_sets, trail: "TrailIndexTable", params: "TrailIndexParams" = None):
        tp = params if params is not None else trail_index_default_params()
        self._chk(lib().hv_trail_init_batch_dev(self._h, C.byref(tp), n_sets, C.byref(trail)), "hv_trail_init_batch_dev")

    def trail_select_batch_dev(self, n_sets, trail: "TrailIndexTable", table: "TrackTable", cam0: "CameraModel", cam1: "CameraModel",
                               keyframe_dev, full_update_dev, frame_num_dev, time_dev, draws_dev, draws_used_dev, n_poses_dev,
                               pose_index_dev, features_dev, velocities_dev, y_dev, cand_id_dev, n_candidates_dev,
                               params: "TrailIndexParams" = None):
        """hv_trail_select_batch_dev (backend.cpp:793-800, 909-1052): pop and stamp, insert, prune, shuffle, score, filter, gather."""
        tp = params if params is not None else trail_index_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_trail_select_batch_dev(self._h, C.byref(tp), n_sets, C.byref(trail), C.byref(table), C.addressof(cam0),
                                                  C.addressof(cam1) if cam1 is not None else None, p(keyframe_dev), p(full_update_dev),
                                                  p(frame_num_dev), p(time_dev), p(draws_dev), p(draws_used_dev), p(n_poses_dev),
                                                  p(pose_index_dev), p(features_dev), p(velocities_dev), p(y_dev), p(cand_id_dev),
                                                  p(n_candidates_dev)),
                  "hv_trail_select_batch_dev")

    def trail_finish_batch_dev(self, n_sets, trail: "TrailIndexTable", cand_id_dev, n_candidates_dev, status_dev, gate_status_dev,
                               stationary_dev, delete_ids_dev, n_delete_dev, good_frame_dev, n_attempts_dev, n_success_dev,
                               discarded_dev, params: "TrailIndexParams" = None):
        """hv_trail_finish_batch_dev (backend.cpp:1189, 1204-1213, 1240-1243, 1269-1274, 804): marks, blacklist, counters, push."""
        tp = params if params is not None else trail_index_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_trail_finish_batch_dev(self._h, C.byref(tp), n_sets, C.byref(trail), p(cand_id_dev), p(n_candidates_dev),
                                                  p(status_dev), p(gate_status_dev), p(stationary_dev), p(delete_ids_dev),
                                                  p(n_delete_dev), p(good_frame_dev), p(n_attempts_dev), p(n_success_dev),
                                                  p(discarded_dev)),
                  "hv_trail_finish_batch_dev")

    # ---- intensity matching: stereo and successive-frame equalisation ----
    def intensity_init_batch_dev(self, n_sets, state: "IntensityState"):
        """hv_intensity_init_batch_dev: no previous frame, cleared workspace."""
        self._chk(lib().hv_intensity_init_batch_dev(self._h, n_sets, C.byref(state)), "hv_intensity_init_batch_dev")

    def match_intensities_batch_dev(self, params: "IntensityParams", n_sets, width, height, left_dev, left_image_stride, right_dev,
                                    right_image_stride, row_stride, state: "IntensityState", active_dev=0, record_dev=0):
        """hv_match_intensities_batch_dev: one frame of n_sets sequences, in place in the caller's gray buffers (addresses;
        right_dev 0 = mono, active_dev [n_sets] bytes or 0, record_dev [n_sets] hv_intensity_record or 0)."""
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_match_intensities_batch_dev(self._h, C.byref(params), n_sets, width, height, p(left_dev),
                                                       int(left_image_stride), p(right_dev), int(right_image_stride),
                                                       int(row_stride), C.byref(state), p(active_dev), p(record_dev)),
                  "hv_match_intensities_batch_dev")

    def match_intensities(self, l: np.ndarray, r: np.ndarray, weight: float = 1.0) -> np.ndarray:
        """hv_match_intensities: matchIntensities(l, r, weight) on one pair of host images; returns the new r (rows may be strided)."""
        assert l.dtype == np.uint8 and r.dtype == np.uint8 and l.shape == r.shape and l.ndim == 2
        assert l.strides[1] == 1 and r.strides[1] == 1
        out = np.array(r, copy=True, order="C")
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(lib().hv_match_intensities(self._h, l.shape[1], l.shape[0], vp(l), l.strides[0], vp(out), out.strides[0],
                                             float(weight)), "hv_match_intensities")
        return out

    # ---- device std::mt19937 streams: the draws of the RANSAC filters and of the shuffle ----
    def rng_seed_batch_dev(self, n_sets, rng: "RngState", seed: int = 0, seed_dev=0, reset_kind_dev=0):
        """hv_rng_seed_batch_dev: std::mt19937(seed) per set (seed_dev [n_sets] uint32 overrides `seed`); with reset_kind_dev only the
        sets that reset are written."""
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_rng_seed_batch_dev(self._h, n_sets, C.byref(rng), int(seed) & 0xffffffff, p(seed_dev), p(reset_kind_dev)),
                  "hv_rng_seed_batch_dev")

    def rng_draw_batch_dev(self, n_sets, rng: "RngState", n_draws, draws_dev):
        """hv_rng_draw_batch_dev: draws_dev [n_sets][n_draws] = the next raw outputs of each set; the state is not changed."""
        self._chk(lib().hv_rng_draw_batch_dev(self._h, n_sets, C.byref(rng), int(n_draws), C.c_void_p(draws_dev or None)),
                  "hv_rng_draw_batch_dev")

    def rng_advance_batch_dev(self, n_sets, rng: "RngState", count_dev, count_stride, multiplier, max_draws):
        """hv_rng_advance_batch_dev: every set moves on by min(multiplier * clamp(count_dev[s * count_stride], 0, max_draws), max_draws)
        outputs. count_dev is an address: summary.data_ptr() + 4 for the RANSAC2 summary (stride 2, multiplier 2), + 8 for the RANSAC3
        and upright summaries (stride 4, multiplier 3 or 2), draws_used (stride 1, multiplier 1)."""
        self._chk(lib().hv_rng_advance_batch_dev(self._h, n_sets, C.byref(rng), C.c_void_p(count_dev or None), int(count_stride),
                                                 int(multiplier), int(max_draws)), "hv_rng_advance_batch_dev")

    # ---- image ingest (f2): colour -> gray and the undistort / rectify remap in front of the pyramid ----
    def ingest_set_undistort_map(self, camera: int, pix_orig=None, valid=None):
        """pix_orig (h, w, 2) f64 = original-image position of every rectified pixel (None removes the table)."""
        if pix_orig is None:
            self._chk(lib().hv_ingest_set_undistort_map(self._h, camera, None, None), "hv_ingest_set_undistort_map")
            return
        pix = np.ascontiguousarray(pix_orig, np.float64)
        assert pix.shape == (self.params.height, self.params.width, 2), pix.shape
        v = None if valid is None else np.ascontiguousarray(valid, np.uint8)
        self._chk(lib().hv_ingest_set_undistort_map(self._h, camera, pix.ctypes.data_as(C.c_void_p),
                                                    None if v is None else v.ctypes.data_as(C.c_void_p)),
                  "hv_ingest_set_undistort_map")

    def ingest_build(self, slot: int, image: np.ndarray, camera: int = -1):
        """image (h, w) gray or (h, w, 3|4) colour, u8."""
        image = np.ascontiguousarray(image, np.uint8)
        ch = 1 if image.ndim == 2 else image.shape[2]
        assert image.shape[:2] == (self.params.height, self.params.width), image.shape
        self._chk(lib().hv_ingest_build(self._h, slot, _p(image, u8p), image.strides[0], ch, camera), "hv_ingest_build")
        self.synchronize()

    def ingest_build_batch_dev(self, n: int, slots_dev: int, src_dev: int, image_stride: int, row_stride: int,
                               channels: int = 1, camera: int = -1):
        self._chk(lib().hv_ingest_build_batch_dev(self._h, n, C.c_void_p(slots_dev), C.c_void_p(src_dev), image_stride,
                                                  row_stride, channels, camera), "hv_ingest_build_batch_dev")

    def download(self, slot: int, level: int):
        w, h = self.level_sizes[level]
        g = np.empty((h, w), np.uint8)
        d = np.empty((h, w, 2), np.int16)
        self._chk(lib().hv_pyramid_download(self._h, slot, level, _p(g, u8p), _p(d, i16p)), "hv_pyramid_download")
        return g, d

    # -- Lucas-Kanade --
    def klt_track(self, prev_slot, next_slot, prev_xy, next_xy=None, max_iter_override=-1):
        prev_xy = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
        n = prev_xy.shape[0]
        use_init = next_xy is not None
        out = (np.ascontiguousarray(next_xy, np.float32).reshape(-1, 2).copy() if use_init
               else np.zeros_like(prev_xy))
        st = np.zeros(n, np.uint8)
        err = np.zeros(n, np.float32)
        self._chk(lib().hv_klt_track(self._h, prev_slot, next_slot, n, _p(prev_xy, f32p), _p(out, f32p),
                                     _p(st, u8p), _p(err, f32p), int(use_init), max_iter_override), "hv_klt_track")
        return out, st, err

    def optical_flow_compute(self, prev_slot, cur_slot, prev_corners, corners=None, override_max_iterations=-1):
        prev_corners = np.ascontiguousarray(prev_corners, np.float32).reshape(-1, 2)
        n = prev_corners.shape[0]
        use_init = corners is not None
        out = (np.ascontiguousarray(corners, np.float32).reshape(-1, 2).copy() if use_init
               else np.zeros_like(prev_corners))
        st = np.full(n, ST_FAILED_FLOW, np.int32)
        self._chk(lib().hv_optical_flow_compute(self._h, prev_slot, cur_slot, n, _p(prev_corners, f32p),
                                                _p(out, f32p), _p(st, i32p), int(use_init),
                                                override_max_iterations), "hv_optical_flow_compute")
        return out, st

    def klt_track_batch_dev(self, n_pairs, prev_slots_dev, next_slots_dev, pts_per_pair, prev_xy_dev,
                            next_xy_dev, status_dev, err_dev, use_initial_flow=True, max_iter_override=-1):
        self._chk(lib().hv_klt_track_batch_dev(self._h, n_pairs, C.c_void_p(prev_slots_dev),
                                               C.c_void_p(next_slots_dev), pts_per_pair, C.c_void_p(prev_xy_dev),
                                               C.c_void_p(next_xy_dev), C.c_void_p(status_dev),
                                               C.c_void_p(err_dev), int(use_initial_flow), max_iter_override),
                  "hv_klt_track_batch_dev")

    def klt_track_batch_ragged_dev(self, n_pairs, prev_slots_dev, next_slots_dev, pts_per_pair, pts_in_pair_dev, prev_xy_dev,
                                   next_xy_dev, status_dev, err_dev, use_initial_flow=True, max_iter_override=-1):
        self._chk(lib().hv_klt_track_batch_ragged_dev(self._h, n_pairs, C.c_void_p(prev_slots_dev), C.c_void_p(next_slots_dev),
                                                      pts_per_pair, C.c_void_p(pts_in_pair_dev), C.c_void_p(prev_xy_dev),
                                                      C.c_void_p(next_xy_dev), C.c_void_p(status_dev), C.c_void_p(err_dev),
                                                      int(use_initial_flow), max_iter_override), "hv_klt_track_batch_ragged_dev")

    # -- GFTT feature detector --
    def gftt_detect(self, slot: int, prev=(), mask_radius: int = 0, params: "GfttParams" = None):
        """FeatureDetector::detect on the level-0 image of a built pyramid slot -> corners [n, 2]."""
        gp = params if params is not None else gftt_default_params()
        nk = lib().hv_gftt_keypoint_count(self._h, C.byref(gp))
        out = np.zeros((max(2 * nk, 1), 2), np.float32)
        pv = np.ascontiguousarray(prev, np.float32).reshape(-1, 2)
        n = C.c_int(0)
        self._chk(lib().hv_gftt_detect(self._h, C.byref(gp), slot, _p(pv, f32p) if len(pv) else None, len(pv),
                                       int(mask_radius), _p(out, f32p), 2 * nk, C.byref(n)), "hv_gftt_detect")
        return out[:n.value].copy()

    def gftt_keypoint_count(self, params: "GfttParams" = None) -> int:
        gp = params if params is not None else gftt_default_params()
        return int(lib().hv_gftt_keypoint_count(self._h, C.byref(gp)))

    def gftt_keypoints_batch_dev(self, n_images: int, slots_dev: int, kp_dev: int, params: "GfttParams" = None):
        gp = params if params is not None else gftt_default_params()
        self._chk(lib().hv_gftt_keypoints_batch_dev(self._h, C.byref(gp), n_images, C.c_void_p(slots_dev),
                                                    C.c_void_p(kp_dev)), "hv_gftt_keypoints_batch_dev")

    def apply_min_distance_batch_dev(self, n_sets, max_corners, n_corners_dev, corners_dev, max_prev, n_prev_dev, prev_dev, radius_dev,
                                     max_tracks, n_out_dev):
        """hv_apply_min_distance_batch_dev: corners_dev [n_sets][max_corners][2] filtered in place, counts in n_out_dev."""
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_apply_min_distance_batch_dev(self._h, n_sets, max_corners, p(n_corners_dev), p(corners_dev), max_prev,
                                                        p(n_prev_dev), p(prev_dev), p(radius_dev), int(max_tracks), p(n_out_dev)),
                  "hv_apply_min_distance_batch_dev")

    def gftt_corners_batch_dev(self, n_images, kp_dev, max_prev, n_prev_dev, prev_dev, mask_radius_dev, max_corners, corners_dev,
                               n_out_dev, params: "GfttParams" = None):
        """hv_gftt_corners_batch_dev: the tail of detect() on the key points of gftt_keypoints_batch_dev."""
        gp = params if params is not None else gftt_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_gftt_corners_batch_dev(self._h, C.byref(gp), n_images, p(kp_dev), max_prev, p(n_prev_dev), p(prev_dev),
                                                  p(mask_radius_dev), max_corners, p(corners_dev), p(n_out_dev)),
                  "hv_gftt_corners_batch_dev")

    def gftt_detect_batch_dev(self, n_images, slots_dev, kp_dev, max_prev, n_prev_dev, prev_dev, mask_radius_dev, max_corners,
                              corners_dev, n_out_dev, params: "GfttParams" = None):
        """hv_gftt_detect_batch_dev: gftt_keypoints_batch_dev + gftt_corners_batch_dev on the context stream."""
        gp = params if params is not None else gftt_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_gftt_detect_batch_dev(self._h, C.byref(gp), n_images, p(slots_dev), p(kp_dev), max_prev, p(n_prev_dev),
                                                 p(prev_dev), p(mask_radius_dev), max_corners, p(corners_dev), p(n_out_dev)),
                  "hv_gftt_detect_batch_dev")

    def gftt_sqrt_dev(self, x_dev: int, y_dev: int, n: int, wide: bool = False):
        """y[i] = the detector's correctly rounded square root of x[i], binary32 device arrays (hv_debug_gftt_sqrt: a debug export
        outside the header, for the tests of the helper); wide: the four-at-once form of the marching kernel."""
        fn = lib().hv_debug_gftt_sqrt
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int]
        self._chk(fn(self._h, C.c_void_p(x_dev), C.c_void_p(y_dev), int(n), int(bool(wide))), "hv_debug_gftt_sqrt")

    # -- FAST feature detector --
    def fast_keypoint_bound(self) -> int:
        """hv_fast_keypoint_bound: a max_keypoints no image of this context can exceed."""
        return int(lib().hv_fast_keypoint_bound(self._h))

    def fast_work_bytes(self, n_images: int) -> int:
        return int(lib().hv_fast_work_bytes(self._h, int(n_images)))

    def fast_detect(self, slot: int, prev=(), mask_radius: int = 1, params: "FastParams" = None):
        """FeatureDetector::detect of the FAST detector on the level-0 image of a built pyramid slot -> corners [n, 2]."""
        fp = params if params is not None else fast_default_params()
        cap = max(min(fp.maxTracks, self.fast_keypoint_bound()), 0)
        out = np.zeros((max(cap, 1), 2), np.float32)
        pv = np.ascontiguousarray(prev, np.float32).reshape(-1, 2)
        n = C.c_int(0)
        self._chk(lib().hv_fast_detect(self._h, C.byref(fp), slot, _p(pv, f32p) if len(pv) else None, len(pv), int(mask_radius),
                                       _p(out, f32p), cap, C.byref(n)), "hv_fast_detect")
        return out[:n.value].copy()

    def fast_keypoints_batch_dev(self, n_images, slots_dev, work_dev, max_keypoints, kp_dev, n_kp_dev, params: "FastParams" = None):
        """hv_fast_keypoints_batch_dev: kp_dev [n_images][max_keypoints][3] = (x, y, score) in row-major order, counts in n_kp_dev."""
        fp = params if params is not None else fast_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_fast_keypoints_batch_dev(self._h, C.byref(fp), n_images, p(slots_dev), p(work_dev), max_keypoints, p(kp_dev),
                                                    p(n_kp_dev)), "hv_fast_keypoints_batch_dev")

    def fast_detect_batch_dev(self, n_images, slots_dev, work_dev, max_keypoints, kp_dev, n_kp_dev, max_prev, n_prev_dev, prev_dev,
                              mask_radius_dev, max_corners, corners_dev, n_out_dev, params: "FastParams" = None):
        """hv_fast_detect_batch_dev: score map, track mask, stable sort by score and the min-distance walk on the context stream."""
        fp = params if params is not None else fast_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_fast_detect_batch_dev(self._h, C.byref(fp), n_images, p(slots_dev), p(work_dev), max_keypoints, p(kp_dev),
                                                 p(n_kp_dev), max_prev, p(n_prev_dev), p(prev_dev), p(mask_radius_dev), max_corners,
                                                 p(corners_dev), p(n_out_dev)), "hv_fast_detect_batch_dev")

    # -- legacy GFTT feature detector (cv::goodFeaturesToTrack behind the track mask) --
    def gftt_legacy_min_distance(self, params: "GfttLegacyParams" = None) -> float:
        """hv_gftt_legacy_min_distance: gfttMinDistance * (min(w, h) / 720.0), binary64."""
        gp = params if params is not None else gftt_legacy_default_params()
        return float(lib().hv_gftt_legacy_min_distance(self._h, C.byref(gp)))

    def gftt_legacy_keypoint_bound(self) -> int:
        """hv_gftt_legacy_keypoint_bound: a max_keypoints no image of this context can exceed."""
        return int(lib().hv_gftt_legacy_keypoint_bound(self._h))

    def gftt_legacy_work_bytes(self, n_images: int, max_keypoints: int) -> int:
        return int(lib().hv_gftt_legacy_work_bytes(self._h, int(n_images), int(max_keypoints)))

    def gftt_legacy_detect(self, slot: int, prev=(), mask_radius: int = 1, params: "GfttLegacyParams" = None):
        """MaskedFeatureDetector::detect of the GFTT detector on the level-0 image of a built pyramid slot -> corners [n, 2]."""
        gp = params if params is not None else gftt_legacy_default_params()
        cap = max(min(gp.maxTracks, self.gftt_legacy_keypoint_bound()), 0)
        out = np.zeros((max(cap, 1), 2), np.float32)
        pv = np.ascontiguousarray(prev, np.float32).reshape(-1, 2)
        n = C.c_int(0)
        self._chk(lib().hv_gftt_legacy_detect(self._h, C.byref(gp), slot, _p(pv, f32p) if len(pv) else None, len(pv), int(mask_radius),
                                              _p(out, f32p), cap, C.byref(n)), "hv_gftt_legacy_detect")
        return out[:n.value].copy()

    def gftt_legacy_keypoints_batch_dev(self, n_images, slots_dev, work_dev, max_keypoints, n_cand_dev, max_corners, corners_dev,
                                        resp_dev, n_out_dev, params: "GfttLegacyParams" = None):
        """hv_gftt_legacy_keypoints_batch_dev: cv::goodFeaturesToTrack with no mask on the context stream."""
        gp = params if params is not None else gftt_legacy_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_gftt_legacy_keypoints_batch_dev(self._h, C.byref(gp), n_images, p(slots_dev), p(work_dev), max_keypoints,
                                                           p(n_cand_dev), max_corners, p(corners_dev), p(resp_dev), p(n_out_dev)),
                  "hv_gftt_legacy_keypoints_batch_dev")

    def gftt_legacy_detect_batch_dev(self, n_images, slots_dev, work_dev, max_keypoints, n_cand_dev, max_prev, n_prev_dev, prev_dev,
                                     mask_radius_dev, max_corners, corners_dev, resp_dev, n_out_dev, params: "GfttLegacyParams" = None):
        """hv_gftt_legacy_detect_batch_dev: track mask, response, masked maximum, candidates, order and the min-distance walk."""
        gp = params if params is not None else gftt_legacy_default_params()
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_gftt_legacy_detect_batch_dev(self._h, C.byref(gp), n_images, p(slots_dev), p(work_dev), max_keypoints,
                                                        p(n_cand_dev), max_prev, p(n_prev_dev), p(prev_dev), p(mask_radius_dev),
                                                        max_corners, p(corners_dev), p(resp_dev), p(n_out_dev)),
                  "hv_gftt_legacy_detect_batch_dev")

    # -- dense stereo depth --
    def stereo_work_bytes(self, n_sets: int, params: "StereoBmParams" = None) -> int:
        sp = params if params is not None else stereo_bm_default_params(self.params.width)
        return int(lib().hv_stereo_work_bytes(self._h, C.byref(sp), int(n_sets)))

    def stereo_cloud_bound(self, cloud_stride: int = 5) -> int:
        """hv_stereo_cloud_bound: a max_points no cloud of this context can exceed."""
        return self._chk_count(lib().hv_stereo_cloud_bound(self._h, int(cloud_stride)), "hv_stereo_cloud_bound")

    def _chk_count(self, rc, what):
        if rc < 0:
            self._chk(rc, what)
        return int(rc)

    def stereo_disparity(self, left_slot: int, right_slot: int, params: "StereoBmParams" = None):
        """OpenCvStereoDisparity::computeDisparity on the level-0 images of two built slots -> int16 [h, w] (disparity x 16)."""
        sp = params if params is not None else stereo_bm_default_params(self.params.width)
        out = np.zeros((self.params.height, self.params.width), np.int16)
        self._chk(lib().hv_stereo_disparity(self._h, C.byref(sp), int(left_slot), int(right_slot), out.ctypes.data_as(C.c_void_p),
                                            self.params.width), "hv_stereo_disparity")
        return out

    def stereo_track_depth(self, disp, xy, q):
        """getDepth of every point on a host disparity image [h, w] int16 -> float32 [n]."""
        disp = np.ascontiguousarray(disp, np.int16)
        pts = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.zeros(max(len(pts), 1), np.float32)
        qa = (C.c_double * 16)(*np.asarray(q, np.float64).reshape(16))
        self._chk(lib().hv_stereo_track_depth(self._h, len(pts), _p(pts, f32p) if len(pts) else None, disp.ctypes.data_as(C.c_void_p),
                                              disp.shape[1], qa, _p(out, f32p)), "hv_stereo_track_depth")
        return out[:len(pts)].copy()

    def stereo_point_cloud(self, disp, q, cloud_stride: int = 5):
        """computePointCloud on a host disparity image -> float32 [n, 3] in row-major visiting order."""
        disp = np.ascontiguousarray(disp, np.int16)
        cap = self.stereo_cloud_bound(cloud_stride)
        out = np.zeros((max(cap, 1), 3), np.float32)
        n = C.c_int(0)
        qa = (C.c_double * 16)(*np.asarray(q, np.float64).reshape(16))
        self._chk(lib().hv_stereo_point_cloud(self._h, disp.ctypes.data_as(C.c_void_p), disp.shape[1], qa, int(cloud_stride),
                                              _p(out, f32p), cap, C.byref(n)), "hv_stereo_point_cloud")
        return out[:n.value].copy()

    def stereo_disparity_batch_dev(self, n_sets, left_slots_dev, right_slots_dev, work_dev, disp_dev, disp_set_stride, n_valid_dev=0,
                                   params: "StereoBmParams" = None):
        """hv_stereo_disparity_batch_dev: prefilter, block matching and the speckle filter on the context stream."""
        sp = params if params is not None else stereo_bm_default_params(self.params.width)
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_stereo_disparity_batch_dev(self._h, C.byref(sp), n_sets, p(left_slots_dev), p(right_slots_dev), p(work_dev),
                                                      p(disp_dev), int(disp_set_stride), p(n_valid_dev)), "hv_stereo_disparity_batch_dev")

    def filter_speckles_batch_dev(self, n_sets, width, height, disp_dev, set_stride, new_val, max_size, max_diff, work_dev):
        """hv_filter_speckles_batch_dev: cv::filterSpeckles in place on int16 maps of any size."""
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_filter_speckles_batch_dev(self._h, n_sets, width, height, p(disp_dev), int(set_stride), int(new_val),
                                                     int(max_size), int(max_diff), p(work_dev)), "hv_filter_speckles_batch_dev")

    def stereo_track_depth_batch_dev(self, n_sets, max_points, n_points_dev, xy_dev, disp_dev, stride, q, depth_dev):
        """hv_stereo_track_depth_batch_dev: getDepth of every track; q: disparityToDepthQ, 16 row-major doubles."""
        p = lambda x: C.c_void_p(x or None)
        qa = (C.c_double * 16)(*np.asarray(q, np.float64).reshape(16))
        self._chk(lib().hv_stereo_track_depth_batch_dev(self._h, n_sets, max_points, p(n_points_dev), p(xy_dev), p(disp_dev), int(stride),
                                                        qa, p(depth_dev)), "hv_stereo_track_depth_batch_dev")

    def stereo_point_cloud_batch_dev(self, n_sets, disp_dev, stride, q, cloud_stride, max_points, xyz_dev, n_points_dev):
        """hv_stereo_point_cloud_batch_dev: computePointCloud in row-major order; -1 for a set that does not fit."""
        p = lambda x: C.c_void_p(x or None)
        qa = (C.c_double * 16)(*np.asarray(q, np.float64).reshape(16))
        self._chk(lib().hv_stereo_point_cloud_batch_dev(self._h, n_sets, p(disp_dev), int(stride), qa, int(cloud_stride), max_points,
                                                        p(xyz_dev), p(n_points_dev)), "hv_stereo_point_cloud_batch_dev")

    # -- sub-pixel corner refinement --
    def corner_subpix(self, slot: int, xy, params: "SubpixParams" = None):
        """SubPixelAdjuster::adjust on the level-0 image of a built pyramid slot -> (refined xy [n, 2], position updates [n])."""
        sp = params if params is not None else subpix_default_params()
        out = np.ascontiguousarray(xy, np.float32).reshape(-1, 2).copy()
        it = np.zeros(len(out), np.int32)
        self._chk(lib().hv_corner_subpix(self._h, C.byref(sp), slot, len(out), _p(out, f32p), _p(it, i32p)), "hv_corner_subpix")
        return out, it

    def corner_subpix_batch_dev(self, n_sets: int, slots_dev: int, max_points: int, n_points_dev: int, xy_dev: int,
                                iters_dev: int = 0, params: "SubpixParams" = None):
        sp = params if params is not None else subpix_default_params()
        self._chk(lib().hv_corner_subpix_batch_dev(self._h, C.byref(sp), n_sets, C.c_void_p(slots_dev), max_points,
                                                   C.c_void_p(n_points_dev), C.c_void_p(xy_dev), C.c_void_p(iters_dev or None)),
                  "hv_corner_subpix_batch_dev")

    # -- timers --
    def profile_enable(self, on=True):
        self._chk(lib().hv_profile_enable(self._h, int(on)), "hv_profile_enable")

    def profile_reset(self):
        self._chk(lib().hv_profile_reset(self._h), "hv_profile_reset")

    def profile_read(self, kernel_id: int):
        ms, n = C.c_double(), C.c_longlong()
        self._chk(lib().hv_profile_read(self._h, kernel_id, C.byref(ms), C.byref(n)), "hv_profile_read")
        return ms.value, n.value


def gftt_default_params(**over) -> GfttParams:
    p = GfttParams()
    lib().hv_gftt_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def ransac5_default_params(**over) -> Ransac5Params:
    p = Ransac5Params()
    lib().hv_ransac5_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def upright2p_default_params(**over) -> Upright2pParams:
    p = Upright2pParams()
    lib().hv_upright2p_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def ransac3_default_params(**over) -> Ransac3Params:
    p = Ransac3Params()
    lib().hv_ransac3_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def stereo_gate_default_params(**over) -> StereoGateParams:
    """hv_stereo_gate_default_params; cam0ToCam1 may be given as any 4 x 4 / 16-element array (row-major)."""
    p = StereoGateParams()
    lib().hv_stereo_gate_default_params(C.byref(p))
    for k, v in over.items():
        if k == "cam0ToCam1":
            p.cam0ToCam1[:] = [float(x) for x in np.asarray(v, np.float64).reshape(16)]
        else:
            setattr(p, k, v)
    return p


def track_table_default_params(**over) -> TrackTableParams:
    p = TrackTableParams()
    lib().hv_track_table_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def track_table(**pointers) -> TrackTable:
    """hv_track_table from device addresses by member name (second_xy omitted or 0: mono)."""
    t = TrackTable()
    for k, v in pointers.items():
        setattr(t, k, v or None)
    return t


def trail_index_default_params(**over) -> TrailIndexParams:
    p = TrailIndexParams()
    lib().hv_trail_index_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def flow_predict_default_params(imu_to_camera=None, second_imu_to_camera=None, **over) -> FlowPredictParams:
    """hv_flow_predict_default_params; a given imuToCamera matrix is stored with its inverse (numpy.linalg.inv)."""
    p = FlowPredictParams()
    lib().hv_flow_predict_default_params(C.byref(p))
    for T, name, inv in ((imu_to_camera, "imuToCamera", "cameraToImu"), (second_imu_to_camera, "secondImuToCamera", "secondCameraToImu")):
        if T is not None:
            T = np.asarray(T, np.float64).reshape(4, 4)
            getattr(p, name)[:] = list(T.reshape(16))
            getattr(p, inv)[:] = list(np.linalg.inv(T).reshape(16))
    for k, v in over.items():
        setattr(p, k, v)
    return p


class TrailIndex:
    """hv_trail_index for n_sets sequences: torch tensors on the current device by member name (self.m) and the pointer table
    over them (self.table). Uninitialised until trail_init_batch_dev."""

    def __init__(self, n_sets: int, params: "TrailIndexParams"):
        S, K, M, V = n_sets, params.cameraTrailLength + 1, params.maxTracks, params.maxVisualUpdates
        Cn = 2 if params.useStereo else 1
        i32, f64 = torch.int32, torch.float64
        shapes = dict(n_keyframes=((S,), i32), frame_counter=((S,), i32), kf_row=((S, K), i32), frame_number=((S, K), i32),
                      timestamp=((S, K), f64), col_id=((S, M), i32), col_len=((S, M), i32),
                      image_point=((S, K, M, Cn, 2), torch.float32), norm_point=((S, K, M, Cn, 2), f64),
                      norm_velocity=((S, K, M, Cn, 2), f64), used=((S, K, M), torch.uint8), n_blacklist=((S,), i32),
                      blacklist_ids=((S, M), i32), n_order=((S,), i32), n_skipped=((S,), i32), skipped_pos=((S, M), i32),
                      skipped_id=((S, M), i32), cand_pos=((S, V), i32), cand_col=((S, V), i32))
        self.m = {k: torch.zeros(shape, dtype=dt, device="cuda") for k, (shape, dt) in shapes.items()}
        self.table = TrailIndexTable(*(self.m[k].data_ptr() for k, _ in TrailIndexTable._fields_))


RNG_STATE_WORDS = 624
RNG_MAX_DRAWS = 2048


class Rng:
    """hv_rng for n_sets sequences: mt [n_sets][624] (int32 tensor holding the uint32 words) and pos [n_sets] int32 on `device`, and
    the pointer table over them (self.table). Uninitialised until rng_seed_batch_dev."""

    def __init__(self, n_sets: int, device="cuda"):
        self.n_sets = n_sets
        self.mt = torch.zeros((n_sets, RNG_STATE_WORDS), dtype=torch.int32, device=device)
        self.pos = torch.zeros((n_sets,), dtype=torch.int32, device=device)
        self.table = RngState(self.mt.data_ptr(), self.pos.data_ptr())


def rng_state(n_sets: int, device="cuda") -> Rng:
    """Allocates an hv_rng (the allocator beside session_state and TrailIndex)."""
    return Rng(n_sets, device)


class Intensity:
    """hv_intensity_state for n_sets sequences on `device` (prev_sum / prev_sqsum int64 tensors holding the uint64 sums, has_prev
    int32, hist [n_sets][2][256] int32 holding the uint32 counts), one hv_intensity_record per set (self.record, bytes; records()
    decodes a download) and the pointer table (self.table). Zeroed; hv_intensity_init_batch_dev does the same on the stream."""

    def __init__(self, n_sets: int, device="cuda"):
        self.n_sets = n_sets
        self.prev_sum = torch.zeros((n_sets,), dtype=torch.int64, device=device)
        self.prev_sqsum = torch.zeros((n_sets,), dtype=torch.int64, device=device)
        self.has_prev = torch.zeros((n_sets,), dtype=torch.int32, device=device)
        self.hist = torch.zeros((n_sets, 2, 256), dtype=torch.int32, device=device)
        self.record = torch.zeros((n_sets, C.sizeof(IntensityRecord)), dtype=torch.uint8, device=device)
        self.table = IntensityState(self.prev_sum.data_ptr(), self.prev_sqsum.data_ptr(), self.has_prev.data_ptr(), self.hist.data_ptr())

    def records(self):
        """The records as a list of IntensityRecord (synchronising download)."""
        raw = self.record.cpu().numpy().tobytes()
        n = C.sizeof(IntensityRecord)
        return [IntensityRecord.from_buffer_copy(raw[i * n:(i + 1) * n]) for i in range(self.n_sets)]


def intensity_state(n_sets: int, device="cuda") -> Intensity:
    """Allocates an hv_intensity_state and its records (the allocator beside rng_state)."""
    return Intensity(n_sets, device)


def intensity_default_params(**over) -> IntensityParams:
    p = IntensityParams()
    lib().hv_intensity_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def fast_default_params(**over) -> FastParams:
    p = FastParams()
    lib().hv_fast_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def fast_tile_size() -> tuple:
    """(width, height) of the FAST score kernel's tile, as the library was built (hv_fast_tile_size)."""
    w, h = C.c_int(), C.c_int()
    lib().hv_fast_tile_size(C.byref(w), C.byref(h))
    return w.value, h.value


def gftt_legacy_default_params(**over) -> GfttLegacyParams:
    p = GfttLegacyParams()
    lib().hv_gftt_legacy_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def gftt_legacy_tile_size() -> tuple:
    """(width, height) of the legacy GFTT kernels' tile, as the library was built (hv_gftt_legacy_tile_size)."""
    w, h = C.c_int(), C.c_int()
    lib().hv_gftt_legacy_tile_size(C.byref(w), C.byref(h))
    return w.value, h.value


def stereo_num_disparities(width: int) -> int:
    return int(lib().hv_stereo_num_disparities(int(width)))


def stereo_bm_default_params(width: int, **over) -> StereoBmParams:
    p = StereoBmParams()
    lib().hv_stereo_bm_default_params(C.byref(p), int(width))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def filter_speckles_work_bytes(width: int, height: int, n_sets: int) -> int:
    return int(lib().hv_filter_speckles_work_bytes(int(width), int(height), int(n_sets)))


STEREO_FILTERED = -16


def subpix_default_params(**over) -> SubpixParams:
    p = SubpixParams()
    lib().hv_subpix_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def apply_min_distance(corners, prev, r: int, max_tracks: int = 200) -> np.ndarray:
    """FeatureDetector::applyMinDistance (host code of the library)."""
    c = np.ascontiguousarray(corners, np.float32).reshape(-1, 2).copy()
    pv = np.ascontiguousarray(prev, np.float32).reshape(-1, 2)
    n = C.c_int(len(c))
    lib().hv_apply_min_distance(_p(c, f32p), C.byref(n), _p(pv, f32p) if len(pv) else None, len(pv), int(r), int(max_tracks))
    return c[:n.value].copy()


def ekf_default_params(**over) -> EkfParams:
    p = EkfParams()
    lib().hv_ekf_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def ekf_control_default_params(**over) -> EkfControlParams:
    p = EkfControlParams()
    lib().hv_ekf_control_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


class EkfControl:
    """hv_ekf_control for `batch` filters: four torch tensors on the current device (zupt_time, init_zupt_time float64;
    was_stationary, frames_since_keyframe int32) and the pointer table over them. Uninitialised until control_init_dev."""

    def __init__(self, batch: int):
        self.zupt_time = torch.empty(batch, dtype=torch.float64, device="cuda")
        self.init_zupt_time = torch.empty(batch, dtype=torch.float64, device="cuda")
        self.was_stationary = torch.empty(batch, dtype=torch.int32, device="cuda")
        self.frames_since_keyframe = torch.empty(batch, dtype=torch.int32, device="cuda")
        self.table = EkfControlTable(*(getattr(self, k).data_ptr() for k, _ in EkfControlTable._fields_))


def session_default_params(**over) -> SessionParams:
    p = SessionParams()
    lib().hv_session_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def session_window(params: SessionParams) -> int:
    """The ring size W of hv_session (backend.cpp:195-197)."""
    return int(float(params.targetFps) / float(params.visualUpdateForEveryNFrame) * params.goodFramesTimeWindowSeconds)


class Session:
    """hv_session for n_sets sequences with a ring of W flags: torch tensors on `device` by member name (self.m) and the pointer
    table over them (self.table). Uninitialised until session_init_dev."""

    def __init__(self, n_sets: int, W: int, device="cuda"):
        S, i32, f64, u8 = n_sets, torch.int32, torch.float64, torch.uint8
        shapes = dict(good_ring=((S, W), torch.float32), ring_head=((S,), i32), ring_entries=((S,), i32), tracking_status=((S,), i32),
                      control_status=((S,), i32), last_reset_time=((S,), f64), first_sample=((S,), u8), first_sample_t=((S,), f64),
                      prev_sample_t=((S,), f64), time=((S,), f64), initialized_orientation=((S,), u8))
        self.n_sets, self.W = n_sets, W
        self.m = {k: torch.zeros(shape, dtype=dt, device=device) for k, (shape, dt) in shapes.items()}
        self.table = SessionState(*(self.m[k].data_ptr() for k, _ in SessionState._fields_))


def session_state(n_sets: int, W: int, device="cuda") -> Session:
    """Allocates an hv_session (the allocator beside track_table and TrailIndex)."""
    return Session(n_sets, W, device)


def output_default_params(imu_to_camera=None, imu_to_output=None, **over) -> OutputParams:
    """hv_output_default_params; the two matrices row-major 4 x 4."""
    p = OutputParams()
    lib().hv_output_default_params(C.byref(p))
    for T, name in ((imu_to_camera, "imuToCamera"), (imu_to_output, "imuToOutput")):
        if T is not None:
            getattr(p, name)[:] = list(np.asarray(T, np.float64).reshape(16))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def output_frame(**pointers) -> OutputFrame:
    """hv_output_frame from device pointers by member name (0 / None = NULL)."""
    f = OutputFrame()
    for k, v in pointers.items():
        setattr(f, k, v or None)
    return f


class Output:
    """hv_output for n_sets sequences: torch tensors on the current device by member name (self.m) and the pointer table over
    them (self.table). T = cameraTrailLength, V = maxVisualUpdates of the parameters."""

    def __init__(self, n_sets: int, params: "OutputParams"):
        S, T, V = n_sets, params.cameraTrailLength, params.maxVisualUpdates
        i32, f64 = torch.int32, torch.float64
        shapes = dict(t=((S,), f64), tracking_status=((S,), i32), stationary_visual=((S,), torch.uint8), inertial_mean=((S, 20), f64),
                      inertial_cov_diag=((S, 20), f64), position_cov=((S, 3, 3), f64), velocity_cov=((S, 3, 3), f64), n_trail=((S,), i32),
                      trail_time=((S, T), f64), trail_pose=((S, T, 7), f64), api_pose=((S, 7), f64), api_trail_pose=((S, T, 7), f64),
                      n_points=((S,), i32), point_id=((S, V), i32), point_status=((S, V), i32),
                      point_first_pixel=((S, V, 2), torch.float32), point_xyz=((S, V, 3), f64))
        self.m = {k: torch.zeros(shape, dtype=dt, device="cuda") for k, (shape, dt) in shapes.items()}
        self.table = OutputTable(*(self.m[k].data_ptr() for k, _ in OutputTable._fields_))


def full_cloud_frame(**pointers) -> FullCloudFrame:
    """hv_full_cloud_frame from device pointers by member name (0 / None = NULL)."""
    f = FullCloudFrame()
    for k, v in pointers.items():
        setattr(f, k, v or None)
    return f


class FullCloud:
    """hv_full_cloud for n_sets sequences: torch tensors on the current device by member name (self.m) and the pointer table over
    them (self.table). M = maxTracks of the index parameters; tail_pose_mask is an int64 tensor holding the 64-bit masks.
    counters=False leaves the optional n_attempts / good_frame NULL."""

    def __init__(self, n_sets: int, params: "TrailIndexParams", counters: bool = True, fill: int = 0):
        S, M = n_sets, params.maxTracks
        i32 = torch.int32
        shapes = dict(n_points=((S,), i32), point_id=((S, M), i32), point_status=((S, M), i32),
                      point_first_pixel=((S, M, 2), torch.float32), point_xyz=((S, M, 3), torch.float64), n_tail=((S,), i32),
                      tail_id=((S, M), i32), tail_status=((S, M), i32), tail_col=((S, M), i32), tail_pose_mask=((S, M), torch.int64),
                      n_attempts=((S,), i32), good_frame=((S,), torch.uint8))
        self.m = {k: torch.full(shape, fill, dtype=dt, device="cuda") for k, (shape, dt) in shapes.items()}
        self.table = FullCloudTable(*(self.m[k].data_ptr() if counters or k not in ("n_attempts", "good_frame") else None
                                      for k, _ in FullCloudTable._fields_))


def _f(a):
    return np.ascontiguousarray(a, np.float64)


class CameraModel(C.Structure):
    """hv_camera_model (tracker::Camera, camera.cpp)."""
    _fields_ = [("kind", C.c_int), ("fx", C.c_double), ("fy", C.c_double), ("ppx", C.c_double), ("ppy", C.c_double),
                ("n_coeffs", C.c_int), ("coeffs", C.c_double * 4), ("rotation_enabled", C.c_int), ("rotation", C.c_double * 9),
                ("max_valid_fov_deg", C.c_double), ("distortion_enabled", C.c_int), ("kinv", C.c_double * 9),
                ("max_theta", C.c_double), ("max_r", C.c_double), ("n_table", C.c_int), ("table", C.c_double * 50)]


def camera_model(kind, fx, fy, ppx, ppy, coeffs=(), rotation=None, max_valid_fov_deg=180.0) -> CameraModel:
    m = CameraModel()
    m.kind = {"pinhole": 0, "fisheye": 1}[kind]
    m.fx, m.fy, m.ppx, m.ppy = fx, fy, ppx, ppy
    m.n_coeffs = len(coeffs)
    for i, c in enumerate(coeffs):
        m.coeffs[i] = c
    if rotation is not None:
        m.rotation_enabled = 1
        m.rotation[:] = list(np.asarray(rotation, np.float64).reshape(9))
    m.max_valid_fov_deg = max_valid_fov_deg
    rc = lib().hv_camera_model_init(C.byref(m))
    if rc != 0:
        raise HvError(f"hv_camera_model_init: {lib().hv_status_string(rc).decode()}")
    return m


class VuParams(C.Structure):
    """hv_vu_params (field names = the reference's parameters)."""
    _fields_ = [("triangulationConvergenceThreshold", C.c_double), ("triangulationConvergenceR", C.c_double),
                ("triangulationRcondThreshold", C.c_double), ("triangulationGaussNewtonIterations", C.c_uint),
                ("triangulationMinDist", C.c_double), ("triangulationMaxDist", C.c_double),
                ("estimateImuCameraTimeShift", C.c_int), ("useStereo", C.c_int),
                ("imuToCamera", C.c_double * 16), ("secondImuToCamera", C.c_double * 16),
                ("useLinearTriangulation", C.c_int),
                ("trackRmseThreshold", C.c_double), ("trackOutlierThresholdGrowthFactor", C.c_double)]


def vu_default_params(imu_to_camera=None, second_imu_to_camera=None, **over) -> VuParams:
    p = VuParams()
    lib().hv_vu_default_params(C.byref(p))
    if imu_to_camera is not None:
        p.imuToCamera[:] = list(np.asarray(imu_to_camera, np.float64).reshape(16))
    if second_imu_to_camera is not None:
        p.secondImuToCamera[:] = list(np.asarray(second_imu_to_camera, np.float64).reshape(16))
        p.useStereo = 1
    for k, v in over.items():
        setattr(p, k, v)
    return p


class Lanes:
    """hv_lanes: n batched contexts of one GPU whose streams come from the device's high-priority queue pool, so that their launch
    chains run beside each other whatever the process did before (include/hybvio_hip.h). ctx[i] are Context objects the set owns."""

    def __init__(self, n_lanes, **kw):
        L = lib()
        p = Params()
        L.hv_default_params(C.byref(p))
        vals = dict(width=752, height=480, levels=4, win=31, max_iter=20, eps=0.03, min_eig=1e-3, max_tracks=200, pool_size=16,
                    max_pairs=1, device=0)
        vals.update(kw)
        for k, v in vals.items():
            setattr(p, k, v)
        self._g = C.c_void_p()
        rc = L.hv_lanes_create(C.byref(p), int(n_lanes), C.byref(self._g))
        if rc != 0:
            self._g = None
            raise HvError(f"hv_lanes_create: {L.hv_status_string(rc).decode()}")
        n = L.hv_lanes_count(self._g)
        kw2 = {k: getattr(p, k) for k in ("width", "height", "levels", "win", "max_iter", "eps", "min_eig", "max_tracks", "pool_size", "max_pairs", "device")}
        self.ctx = [Context(_adopt=L.hv_lanes_ctx(self._g, i), **kw2) for i in range(n)]

    def close(self):
        if getattr(self, "_g", None):
            for c in self.ctx:
                c.close()                             # (closes the lanes' hv_ekf children; the contexts themselves die with the set)
            lib().hv_lanes_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:                             # interpreter shutdown: module globals may be gone already
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class EkfBatch:
    """hv_ekf: a batch of independent filters on one Context (batch = 1: the reference's EKF)."""

    def __init__(self, ctx: Context, params: EkfParams | None = None, batch: int = 1):
        self.ctx, self.batch = ctx, batch
        self.params = params if params is not None else ekf_default_params()
        self._h = C.c_void_p()
        rc = lib().hv_ekf_create(ctx._h, C.byref(self.params), batch, C.byref(self._h))
        if rc != 0:
            self._h = None
            raise HvError(f"hv_ekf_create: {lib().hv_status_string(rc).decode()}")
        self.n = lib().hv_ekf_state_dim(self._h)
        if not hasattr(ctx, "_children"):
            ctx._children = []
        ctx._children.append(self)

    def close(self):
        if getattr(self, "_h", None):
            lib().hv_ekf_destroy(self._h)
            self._h = None
            if self in getattr(self.ctx, "_children", []):
                self.ctx._children.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:                             # interpreter shutdown: module globals may be gone already
            pass

    def _chk(self, rc, what):
        self.ctx._chk(rc, what)

    def frame_error(self) -> int:
        """Reads and clears the device error word of the batch (hv_ekf_frame_error)."""
        v = C.c_int()
        self._chk(lib().hv_ekf_frame_error(self._h, C.byref(v)), "hv_ekf_frame_error")
        return v.value

    def set_state(self, b, m=None, P=None):
        mm = _f(m) if m is not None else None
        PP = np.asfortranarray(P, np.float64) if P is not None else None
        self._chk(lib().hv_ekf_set_state(self._h, b, _p(mm, f64p), PP.ctypes.data_as(f64p) if PP is not None else None),
                  "hv_ekf_set_state")

    def get_state(self, b):
        m, P = np.zeros(self.n), np.zeros((self.n, self.n))
        self._chk(lib().hv_ekf_get_state(self._h, b, _p(m, f64p), _p(P, f64p)), "hv_ekf_get_state")
        return m, P.T.copy()          # column-major buffer -> P[i, j]

    def get_means(self):
        m = np.zeros((self.batch, self.n))
        self._chk(lib().hv_ekf_get_means(self._h, _p(m, f64p)), "hv_ekf_get_means")
        return m

    def set_process_noise(self, b, Q):
        self._chk(lib().hv_ekf_set_process_noise(self._h, b, np.asfortranarray(Q, np.float64).ctypes.data_as(f64p)),
                  "hv_ekf_set_process_noise")

    def get_dydx(self, b):
        F = np.zeros((20, 20))
        self._chk(lib().hv_ekf_get_dydx(self._h, b, _p(F, f64p)), "hv_ekf_get_dydx")
        return F.T.copy()

    def device_pointers(self):
        m, P = C.c_void_p(), C.c_void_p()
        self._chk(lib().hv_ekf_device_pointers(self._h, C.byref(m), C.byref(P)), "hv_ekf_device_pointers")
        return m.value, P.value

    def predict(self, dt, gyro, acc):
        dt, gyro, acc = _f(np.broadcast_to(dt, (self.batch,))), _f(np.broadcast_to(gyro, (self.batch, 3))), _f(np.broadcast_to(acc, (self.batch, 3)))
        self._chk(lib().hv_ekf_predict(self._h, _p(dt, f64p), _p(gyro, f64p), _p(acc, f64p)), "hv_ekf_predict")
        self.ctx.synchronize()

    def predict_n_dev(self, n_samples, dt_dev, gyro_dev, acc_dev):
        """n_samples predicts in one launch; device arrays [n][batch], [n][batch][3], [n][batch][3]."""
        self._chk(lib().hv_ekf_predict_n_dev(self._h, int(n_samples), C.c_void_p(dt_dev), C.c_void_p(gyro_dev),
                                             C.c_void_p(acc_dev)), "hv_ekf_predict_n_dev")

    def predict_dev(self, dt_dev, gyro_dev, acc_dev):
        self._chk(lib().hv_ekf_predict_dev(self._h, C.c_void_p(dt_dev), C.c_void_p(gyro_dev), C.c_void_p(acc_dev)),
                  "hv_ekf_predict_dev")

    @staticmethod
    def _pack_H(H, batch):
        H = np.asarray(H, np.float64)
        if H.ndim == 2:
            H = np.broadcast_to(H, (batch,) + H.shape)
        nr, l = H.shape[1:]
        return np.ascontiguousarray(np.transpose(H, (0, 2, 1))), nr, l     # [b][col][row] == column-major per filter

    def update(self, H, y, r_diag, active=None, normalize_all=False):
        Hc, nr, l = self._pack_H(H, self.batch)
        y = _f(np.broadcast_to(y, (self.batch, nr)))
        rd = _f(np.broadcast_to(r_diag, (self.batch,)))
        act = np.ascontiguousarray(active, np.uint8) if active is not None else None
        self._chk(lib().hv_ekf_update(self._h, nr, l, _p(Hc, f64p), _p(y, f64p), _p(rd, f64p), _p(act, u8p),
                                      int(normalize_all)), "hv_ekf_update")
        self.ctx.synchronize()

    def visual_gate(self, H, v, r):
        Hc, nr, l = self._pack_H(H, self.batch)
        v = _f(np.broadcast_to(v, (self.batch, nr)))
        chi2, st = np.zeros(self.batch), np.zeros(self.batch, np.int32)
        self._chk(lib().hv_ekf_visual_gate(self._h, nr, l, _p(Hc, f64p), _p(v, f64p), r, _p(chi2, f64p), _p(st, i32p)),
                  "hv_ekf_visual_gate")
        return chi2, st

    def visual_update(self, H, v, r, active=None):
        Hc, nr, l = self._pack_H(H, self.batch)
        v = _f(np.broadcast_to(v, (self.batch, nr)))
        act = np.ascontiguousarray(active, np.uint8) if active is not None else None
        self._chk(lib().hv_ekf_visual_update(self._h, nr, l, _p(Hc, f64p), _p(v, f64p), r, _p(act, u8p)),
                  "hv_ekf_visual_update")
        self.ctx.synchronize()

    def visual_prepare_dev(self, params: VuParams, n_poses, pose_index_dev, features_dev, velocities_dev, y_dev, H_dev, v_dev,
                           f_dev, pf_dev, status_dev, active_dev=0):
        """hv_ekf_visual_prepare_dev: device pointers (ints); y_dev / f_dev / active_dev may be 0."""
        p = [C.c_void_p(x) for x in (pose_index_dev, features_dev, velocities_dev, y_dev, H_dev, v_dev, f_dev, pf_dev, status_dev, active_dev)]
        self._chk(lib().hv_ekf_visual_prepare_dev(self._h, C.byref(params), n_poses, *p), "hv_ekf_visual_prepare_dev")

    def visual_track_dev(self, params: VuParams, n_poses, pose_index_dev, features_dev, velocities_dev, y_dev, r_gate, r_update,
                         status_dev, gate_status_dev, chi2_dev=0, pf_dev=0):
        a = [C.c_void_p(x) for x in (pose_index_dev, features_dev, velocities_dev, y_dev)]
        b = [C.c_void_p(x) for x in (status_dev, gate_status_dev, chi2_dev, pf_dev)]
        self._chk(lib().hv_ekf_visual_track_dev(self._h, C.byref(params), n_poses, *a, float(r_gate), float(r_update), *b),
                  "hv_ekf_visual_track_dev")

    def visual_track_hybrid_dev(self, params: VuParams, n_poses, pose_index_dev, features_dev, velocities_dev, y_dev, map_update_dev, map_offer_dev,
                                r_gate, r_update, status_dev, gate_status_dev, chi2_dev=0, pf_dev=0):
        """hv_ekf_visual_track_hybrid_dev: a track visit with hybrid-map tracks (map_update_dev) and map-point offers (map_offer_dev)."""
        a = [C.c_void_p(x) for x in (pose_index_dev, features_dev, velocities_dev, y_dev, map_update_dev, map_offer_dev)]
        b = [C.c_void_p(x) for x in (status_dev, gate_status_dev, chi2_dev, pf_dev)]
        self._chk(lib().hv_ekf_visual_track_hybrid_dev(self._h, C.byref(params), n_poses, *a, float(r_gate), float(r_update), *b),
                  "hv_ekf_visual_track_hybrid_dev")

    def visual_track_limited_dev(self, params: VuParams, n_poses, pose_index_dev, features_dev, velocities_dev, y_dev, r_gate, r_update,
                                 status_dev, gate_status_dev, success_counter_dev, max_successful, chi2_dev=0, pf_dev=0):
        a = [C.c_void_p(x) for x in (pose_index_dev, features_dev, velocities_dev, y_dev)]
        b = [C.c_void_p(x) for x in (status_dev, gate_status_dev, chi2_dev, pf_dev, success_counter_dev)]
        self._chk(lib().hv_ekf_visual_track_limited_dev(self._h, C.byref(params), n_poses, *a, float(r_gate), float(r_update), *b,
                                                        int(max_successful)), "hv_ekf_visual_track_limited_dev")

    def visual_track(self, params: VuParams, pose_index, features, velocities, y, r_gate, r_update):
        """hv_ekf_visual_track with numpy arrays [batch][...]: returns (status [batch][2], gate_status, chi2, pf)."""
        idx = np.ascontiguousarray(pose_index, np.int32).reshape(self.batch, -1)
        ft, vl, yy = _f(features), _f(velocities), _f(y)
        st, gs = np.zeros((self.batch, 2), np.int32), np.zeros(self.batch, np.int32)
        chi, pf = np.zeros(self.batch), np.zeros((self.batch, 3))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._chk(lib().hv_ekf_visual_track(self._h, C.byref(params), idx.shape[1], vp(idx), vp(ft), vp(vl), vp(yy), float(r_gate),
                                            float(r_update), vp(st), vp(gs), vp(chi), vp(pf)), "hv_ekf_visual_track")
        return st, gs, chi, pf

    def visual_dev(self, nr, l, H_dev, v_dev, r, mode, chi2_dev=0, status_dev=0):
        self._chk(lib().hv_ekf_visual_dev(self._h, nr, l, C.c_void_p(H_dev), C.c_void_p(v_dev), r, mode,
                                          C.c_void_p(chi2_dev), C.c_void_p(status_dev)), "hv_ekf_visual_dev")

    def augment(self, discarded=None, active=None):
        d = np.ascontiguousarray(np.broadcast_to(discarded, (self.batch,)), np.int32) if discarded is not None else None
        act = np.ascontiguousarray(active, np.uint8) if active is not None else None
        self._chk(lib().hv_ekf_augment(self._h, _p(d, i32p), _p(act, u8p)), "hv_ekf_augment")
        self.ctx.synchronize()

    def augment_dev(self, discarded_dev=0, active_dev=0):
        """hv_ekf_augment_dev: device arrays (or 0), asynchronous."""
        self._chk(lib().hv_ekf_augment_dev(self._h, C.c_void_p(discarded_dev), C.c_void_p(active_dev)), "hv_ekf_augment_dev")

    def symmetrize_augment_dev(self, discarded_dev=0, active_dev=0):
        """hv_ekf_symmetrize_augment_dev: symmetrize() + augment_dev() in one pass over P, asynchronous."""
        self._chk(lib().hv_ekf_symmetrize_augment_dev(self._h, C.c_void_p(discarded_dev), C.c_void_p(active_dev)), "hv_ekf_symmetrize_augment_dev")

    def visual_frame_dev(self, params: VuParams, n_tracks, n_poses, pose_index_dev, features_dev, velocities_dev, y_dev, r_gate, r_update,
                         status_dev, gate_status_dev, success_counter_dev, max_successful, chi2_dev=0, pf_dev=0):
        """hv_ekf_visual_frame_dev: the whole visual-update loop of a frame, track-major device arrays."""
        a = [C.c_void_p(x) for x in (pose_index_dev, features_dev, velocities_dev, y_dev)]
        b = [C.c_void_p(x) for x in (status_dev, gate_status_dev, chi2_dev, pf_dev, success_counter_dev)]
        self._chk(lib().hv_ekf_visual_frame_dev(self._h, C.byref(params), int(n_tracks), int(n_poses), *a, float(r_gate), float(r_update), *b,
                                                int(max_successful)), "hv_ekf_visual_frame_dev")

    def visual_frame_ragged_dev(self, params: VuParams, n_tracks, n_poses_max, n_poses_dev, pose_index_dev, features_dev, velocities_dev, y_dev,
                                r_gate, r_update, status_dev, gate_status_dev, success_counter_dev, max_successful, chi2_dev=0, pf_dev=0):
        """hv_ekf_visual_frame_ragged_dev: per (visit, filter) track lengths n_poses_dev [n_tracks][batch] (< 2: no track)."""
        a = [C.c_void_p(x) for x in (n_poses_dev, pose_index_dev, features_dev, velocities_dev, y_dev)]
        b = [C.c_void_p(x) for x in (status_dev, gate_status_dev, chi2_dev, pf_dev, success_counter_dev)]
        self._chk(lib().hv_ekf_visual_frame_ragged_dev(self._h, C.byref(params), int(n_tracks), int(n_poses_max), *a, float(r_gate),
                                                       float(r_update), *b, int(max_successful)), "hv_ekf_visual_frame_ragged_dev")

    def visual_frame_batch_dev(self, params: VuParams, n_tracks, n_poses_max, n_poses_dev, pose_index_dev, features_dev, velocities_dev, y_dev,
                               r_gate, r_update, status_dev, gate_status_dev, success_counter_dev, max_successful, max_update_rows=0, chi2_dev=0, pf_dev=0):
        """hv_ekf_visual_frame_batch_dev: the frame loop with batchVisualUpdate (inlier blocks applied as one update per batch)."""
        a = [C.c_void_p(x) for x in (n_poses_dev, pose_index_dev, features_dev, velocities_dev, y_dev)]
        b = [C.c_void_p(x) for x in (status_dev, gate_status_dev, chi2_dev, pf_dev, success_counter_dev)]
        self._chk(lib().hv_ekf_visual_frame_batch_dev(self._h, C.byref(params), int(n_tracks), int(n_poses_max), *a, float(r_gate),
                                                      float(r_update), *b, int(max_successful), int(max_update_rows)), "hv_ekf_visual_frame_batch_dev")

    def visual_frame(self, params: VuParams, pose_index, features, velocities, y, r_gate, r_update, max_successful):
        """hv_ekf_visual_frame with numpy arrays [n_tracks][batch][...]: returns (status [K][B][2], gate_status [K][B], chi2, pf, applied [B])."""
        idx = np.ascontiguousarray(pose_index, np.int32)
        K = idx.shape[0]
        idx = idx.reshape(K, self.batch, -1)
        ft, vl, yy = _f(features), _f(velocities), _f(y)
        st, gs = np.zeros((K, self.batch, 2), np.int32), np.zeros((K, self.batch), np.int32)
        chi, pf, cnt = np.zeros((K, self.batch)), np.zeros((K, self.batch, 3)), np.zeros(self.batch, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._chk(lib().hv_ekf_visual_frame(self._h, C.byref(params), K, idx.shape[2], vp(idx), vp(ft), vp(vl), vp(yy), float(r_gate),
                                            float(r_update), vp(st), vp(gs), vp(chi), vp(pf), vp(cnt), int(max_successful)), "hv_ekf_visual_frame")
        return st, gs, chi, pf, cnt

    def undo_augment(self, active=None):
        act = np.ascontiguousarray(active, np.uint8) if active is not None else None
        self._chk(lib().hv_ekf_undo_augment(self._h, _p(act, u8p)), "hv_ekf_undo_augment")
        self.ctx.synchronize()

    def undo_augment_dev(self, active_dev=0):
        """hv_ekf_undo_augment_dev: the mask as a device array (or 0), asynchronous."""
        self._chk(lib().hv_ekf_undo_augment_dev(self._h, C.c_void_p(active_dev)), "hv_ekf_undo_augment_dev")

    def block_update_dev(self, col0, rows, y_dev=0, r_dev=0, r0=0.0, active_dev=0, normalize_all=False, applied_dev=0):
        """hv_ekf_block_update_dev: the update with `rows` unit rows at state entry col0; R = r I already scaled by noiseScale^2."""
        self._chk(lib().hv_ekf_block_update_dev(self._h, int(col0), int(rows), C.c_void_p(y_dev), C.c_void_p(r_dev), float(r0),
                                                C.c_void_p(active_dev), int(normalize_all), C.c_void_p(applied_dev)), "hv_ekf_block_update_dev")

    def pseudo_velocity_dev(self, limit, target, r, active_dev=0, applied_dev=0):
        self._chk(lib().hv_ekf_pseudo_velocity_dev(self._h, float(limit), float(target), float(r), C.c_void_p(active_dev),
                                                   C.c_void_p(applied_dev)), "hv_ekf_pseudo_velocity_dev")

    def control_init_dev(self, ctl: "EkfControl"):
        self._chk(lib().hv_ekf_control_init_dev(self._h, C.byref(ctl.table)), "hv_ekf_control_init_dev")

    def imu_control_dev(self, params: "EkfControlParams", ctl: "EkfControl", time_dev, active_dev=0):
        """hv_ekf_imu_control_dev: init-ZUPT then pseudo-velocity behind a predict; time_dev [batch] float64."""
        self._chk(lib().hv_ekf_imu_control_dev(self._h, C.byref(params), C.byref(ctl.table), C.c_void_p(time_dev), C.c_void_p(active_dev)),
                  "hv_ekf_imu_control_dev")

    def frame_control_dev(self, params: "EkfControlParams", ctl: "EkfControl", time_dev, keyframe_dev, full_update_dev=0, keyframe_out_dev=0,
                          undo_active_dev=0, stationary_dev=0, applied_dev=0):
        """hv_ekf_frame_control_dev: the frame's keyframe counter, visual-stationarity ZUPT and undo mask."""
        a = [C.c_void_p(x) for x in (time_dev, keyframe_dev, full_update_dev, keyframe_out_dev, undo_active_dev, stationary_dev, applied_dev)]
        self._chk(lib().hv_ekf_frame_control_dev(self._h, C.byref(params), C.byref(ctl.table), *a), "hv_ekf_frame_control_dev")

    def session_init_dev(self, params: "SessionParams", st: "Session"):
        """hv_session_init_dev: a Control and its first Session; the filter is not touched."""
        self._chk(lib().hv_session_init_dev(self._h, C.byref(params), C.byref(st.table)), "hv_session_init_dev")

    def session_imu_dev(self, st: "Session", n_samples, t_dev, acc_dev, dt_dev, time_dev, active_dev=0):
        """hv_session_imu_dev: orientation on the first sample and the sample clock; t_dev, dt_dev, time_dev [n][batch], acc_dev [n][batch][3]."""
        a = [C.c_void_p(x) for x in (t_dev, acc_dev, active_dev, dt_dev, time_dev)]
        self._chk(lib().hv_session_imu_dev(self._h, C.byref(st.table), int(n_samples), *a), "hv_session_imu_dev")

    def session_status_dev(self, params: "SessionParams", st: "Session", good_frame_dev, reset_kind_dev, full_update_dev=0, status_dev=0,
                           frozen_dev=0):
        """hv_session_status_dev: the good-frame ring, the tracking status and the reset decision of a frame."""
        a = [C.c_void_p(x) for x in (good_frame_dev, full_update_dev, status_dev, frozen_dev, reset_kind_dev)]
        self._chk(lib().hv_session_status_dev(self._h, C.byref(params), C.byref(st.table), *a), "hv_session_status_dev")

    def session_reset_dev(self, params: "SessionParams", st: "Session", ctl: "EkfControl", tracks_params: "TrackTableParams",
                          table: "TrackTable", trail_params: "TrailIndexParams", trail: "TrailIndexTable", reset_kind_dev):
        """hv_session_reset_dev: Control::reset in place for the sets whose reset kind is 1 (fresh) or 2 (keep the pose)."""
        self._chk(lib().hv_session_reset_dev(self._h, C.byref(params), C.byref(st.table), C.byref(ctl.table), C.byref(tracks_params),
                                             C.byref(table), C.byref(trail_params), C.byref(trail), C.c_void_p(reset_kind_dev)),
                  "hv_session_reset_dev")

    def output_dev(self, params: "OutputParams", st: "Session", trail: "TrailIndexTable", frame: "OutputFrame", out: "Output"):
        """hv_output_dev: the frame's output record of every set (pose, covariances, pose trail, status, point cloud)."""
        self._chk(lib().hv_output_dev(self._h, C.byref(params), C.byref(st.table), C.byref(trail), C.byref(frame), C.byref(out.table)),
                  "hv_output_dev")

    def full_point_cloud_dev(self, trail_params: "TrailIndexParams", vu_params: "VuParams", trail: "TrailIndexTable", table: "TrackTable",
                             frame: "FullCloudFrame", out: "FullCloud"):
        """hv_full_point_cloud_dev (odometry.fullPointCloud): the cloud of the visited tracks with the stopping candidate, then every
        remaining track of the shuffled order, triangulated from the mean as the frame's updates left it. Between
        visual_frame_ragged_dev and trail_finish_batch_dev."""
        self._chk(lib().hv_full_point_cloud_dev(self._h, C.byref(trail_params), C.byref(vu_params), C.byref(trail), C.byref(table),
                                                C.byref(frame), C.byref(out.table)), "hv_full_point_cloud_dev")

    def flow_predict_batch_dev(self, params: "FlowPredictParams", kind: int, trail_params: "TrailIndexParams", trail: "TrailIndexTable",
                               table: "TrackTable", c0_dev, cam0: "CameraModel", cam1: "CameraModel", pred_xy_dev, distance_dev=0,
                               reuse_distance=False):
        """hv_flow_predict_batch_dev (backend.cpp:545-664): the LK start points of every table track of every filter's sequence.
        kind: FLOW_PREDICT_LEFT / RIGHT / STEREO; cam1 may be None for LEFT; distance_dev 0: not kept."""
        self._chk(lib().hv_flow_predict_batch_dev(self._h, C.byref(params), int(kind), C.byref(trail_params), C.byref(trail), C.byref(table),
                                                  C.c_void_p(c0_dev), C.addressof(cam0), C.addressof(cam1) if cam1 is not None else None,
                                                  C.c_void_p(pred_xy_dev), C.c_void_p(distance_dev), int(bool(reuse_distance))),
                  "hv_flow_predict_batch_dev")

    def upright2p_lk_batch_dev(self, cam_params: "FlowPredictParams", max_points, n_points_dev, prev_left_dev, prev_right_dev,
                               cur_left_dev, track_status_dev, r2_summary_dev, cam0: "CameraModel", cam1: "CameraModel", second_to_first,
                               draws_dev, result_dev, score_dev, model_dev=0, summary_dev=0, params: "Upright2pParams" = None):
        """hv_upright2p_lk_batch_dev: the upright 2-point filter of every filter's sequence (set s is filter s) with the two poses
        formed on the device from the mean (history pose 0 and the current pose through cam_params.cameraToImu)."""
        rp = params if params is not None else upright2p_default_params()
        T = np.ascontiguousarray(second_to_first, np.float64).reshape(16)
        p = lambda x: C.c_void_p(x or None)
        self._chk(lib().hv_upright2p_lk_batch_dev(self._h, C.byref(rp), C.byref(cam_params), max_points, p(n_points_dev), p(prev_left_dev),
                                                  p(prev_right_dev), p(cur_left_dev), p(track_status_dev), p(r2_summary_dev),
                                                  C.addressof(cam0), C.addressof(cam1), T.ctypes.data_as(C.c_void_p), p(draws_dev),
                                                  p(result_dev), p(score_dev), p(model_dev), p(summary_dev)),
                  "hv_upright2p_lk_batch_dev")

    def symmetrize(self):
        self._chk(lib().hv_ekf_symmetrize(self._h), "hv_ekf_symmetrize")

    def normalize_quaternions(self, only_current=False):
        self._chk(lib().hv_ekf_normalize_quaternions(self._h, int(only_current)), "hv_ekf_normalize_quaternions")

    def transform(self, b, pC, qC, tr):
        self._chk(lib().hv_ekf_transform(self._h, b, _p(_f(pC), f64p), _p(_f(qC), f64p), _p(_f(tr), f64p)),
                  "hv_ekf_transform")
        self.ctx.synchronize()


# ---- resident VIO engine (hv_vio_*): one object, one call per frame -------------------------------------------------------
DETECTOR_GPU_GFTT, DETECTOR_FAST, DETECTOR_GFTT = 0, 1, 2
TRACKING_INIT, TRACKING_TRACKING, TRACKING_LOST = 0, 1, 2


class VioParams(C.Structure):
    """hv_vio_params: one member per owned entry, the two cameras and the session's scalars."""
    _fields_ = [("ekf", EkfParams), ("gftt", GfttParams), ("subpix", SubpixParams), ("gate", StereoGateParams), ("ransac3", Ransac3Params),
                ("tracks", TrackTableParams), ("trail", TrailIndexParams), ("flow", FlowPredictParams), ("vu", VuParams),
                ("control", EkfControlParams), ("session", SessionParams), ("output", OutputParams), ("camera0", CameraModel),
                ("camera1", CameraModel), ("ransac2Threshold", C.c_double), ("trackChiTestOutlierR", C.c_double), ("visualR", C.c_double),
                ("ransacRngSeed", C.c_int), ("odometryRngSeed", C.c_int), ("imu_samples_max", C.c_int), ("featureDetector", C.c_int),
                ("useRansac3", C.c_int), ("predictOpticalFlow", C.c_int), ("batchVisualUpdate", C.c_int),
                ("ransac5", Ransac5Params), ("upright2p", Upright2pParams), ("fast", FastParams), ("gftt_legacy", GfttLegacyParams),
                ("useStereoUpright2p", C.c_int), ("useHybridRansac", C.c_int)]


class VioView(C.Structure):
    """hv_vio_view: the owned objects and the device pointers of the frame's stage outputs."""
    _fields_ = [("ekf", C.c_void_p), ("table", TrackTable), ("trail", TrailIndexTable), ("session", SessionState), ("control", EkfControlTable),
                ("rng_pipeline", RngState), ("rng_ransac3", RngState), ("rng_odometry", RngState), ("record", OutputTable)] + [
        (k, C.c_void_p) for k in ("frame_num", "has_previous", "full_update", "keyframe", "keyframe_out", "good_frame", "reset_kind",
                                  "tracking_status", "n_candidates", "cand_id", "status", "gate_status", "slot_prev_left", "slot_cur_left",
                                  "slot_right", "ransac_result", "ransac_score", "r5_summary")]


PROTOTYPES.update({
    "hv_vio_default_params": (None, [C.POINTER(VioParams)]),
    "hv_vio_create": (C.c_int, [C.c_void_p, C.POINTER(VioParams), C.c_int, C.POINTER(C.c_void_p)]),
    "hv_vio_create_session": (C.c_int, [C.c_void_p, C.POINTER(VioParams), C.c_int, C.POINTER(C.c_void_p)]),
    "hv_vio_destroy": (None, [C.c_void_p]),
    "hv_vio_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hv_vio_view_get": (C.c_int, [C.c_void_p, C.POINTER(VioView)]),
    "hv_vio_replay_period": (C.c_int, [C.c_void_p]),
    "hv_vio_sets": (C.c_int, [C.c_void_p]),
})


def vio_default_params(**over) -> VioParams:
    """hv_vio_default_params; an override names a member (ransac2Threshold=3.0) or, with a double underscore, a member of a member
    (tracks__maxTracks=120); matrices take 16 values."""
    p = VioParams()
    lib().hv_vio_default_params(C.byref(p))
    for k, v in over.items():
        obj, names = p, k.split("__")
        for name in names[:-1]:
            obj = getattr(obj, name)
        if isinstance(getattr(obj, names[-1]), C.Array):
            getattr(obj, names[-1])[:] = list(np.asarray(v, np.float64).reshape(-1))
        else:
            setattr(obj, names[-1], v)
    return p


class _Wrapped:
    """A device array the engine owns, as the interface torch.as_tensor reads (no copy)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2)


def _wrap(ptr, shape, typestr):
    return torch.as_tensor(_Wrapped(ptr, shape, typestr), device="cuda")


class VioEngine:
    """hv_vio: a session of n_sets resident sequences on one Context; frame() is one frame of every set. session=False is
    hv_vio_create (the default stereo session, everything else refused); session=True is hv_vio_create_session (mono and stereo, every
    track filter, every detector). A mono session's frame() takes right_dev = 0."""

    def __init__(self, ctx: Context, params: VioParams | None = None, n_sets: int = 1, session: bool = False):
        self.ctx, self.n_sets = ctx, n_sets
        self.params = params if params is not None else vio_default_params()
        self._h = C.c_void_p()
        name = "hv_vio_create_session" if session else "hv_vio_create"
        rc = getattr(lib(), name)(ctx._h, C.byref(self.params), n_sets, C.byref(self._h))
        if rc != 0:
            self._h = None
            ctx._chk(rc, name)
        if not hasattr(ctx, "_children"):
            ctx._children = []
        ctx._children.append(self)

    @classmethod
    def create(cls, ctx: Context, params: VioParams | None = None, n_sets: int = 1, session: bool = False) -> "VioEngine":
        return cls(ctx, params, n_sets, session)

    def close(self):
        if getattr(self, "_h", None):
            lib().hv_vio_destroy(self._h)
            self._h = None
            if self in getattr(self.ctx, "_children", []):
                self.ctx._children.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:                             # interpreter shutdown: module globals may be gone already
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def frame(self, left_dev, right_dev, image_stride, row_stride, n_samples, t_dev, gyro_dev, acc_dev):
        p = lambda x: C.c_void_p(x) if x else None
        self.ctx._chk(lib().hv_vio_frame(self._h, p(left_dev), p(right_dev), image_stride, row_stride, n_samples, p(t_dev), p(gyro_dev),
                                         p(acc_dev)), "hv_vio_frame")

    def replay_period(self) -> int:
        return lib().hv_vio_replay_period(self._h)

    def raw_view(self) -> VioView:
        v = VioView()
        self.ctx._chk(lib().hv_vio_view_get(self._h, C.byref(v)), "hv_vio_view_get")
        return v

    def view(self) -> dict:
        """The engine's arrays as torch tensors over its own device memory (nothing is copied): 'table', 'trail', 'session',
        'control', 'record' and the three 'rng_*' are dicts by member name, the stage outputs are tensors, 'ekf_handle' is the
        engine's hv_ekf (not owned; state() reads its mean and covariance back). An array the session does not have (a mono
        session's table.second_xy and slot_right, r5_summary without the hybrid filter) is None."""
        raw, p, S = self.raw_view(), self.params, self.n_sets
        M, K, V, T = p.tracks.maxTracks, p.trail.cameraTrailLength + 1, p.trail.maxVisualUpdates, p.output.cameraTrailLength
        W = session_window(p.session)
        Cn = 2 if p.trail.useStereo else 1
        i4, f4, f8, u1 = "<i4", "<f4", "<f8", "|u1"
        spec = dict(
            table=dict(n_tracks=((S,), i4), ids=((S, M), i4), xy=((S, M, 2), f4), second_xy=((S, M, 2), f4), status=((S, M), i4),
                       blacklist=((S, M), u1), kf_xy=((S, M, 2), f4), kf_valid=((S, M), u1), frame_num=((S,), i4), mask_steps=((S,), i4),
                       mask_radius=((S,), i4), frame_flags=((S,), u1)),
            trail=dict(n_keyframes=((S,), i4), frame_counter=((S,), i4), kf_row=((S, K), i4), frame_number=((S, K), i4),
                       timestamp=((S, K), f8), col_id=((S, M), i4), col_len=((S, M), i4), image_point=((S, K, M, Cn, 2), f4),
                       norm_point=((S, K, M, Cn, 2), f8), norm_velocity=((S, K, M, Cn, 2), f8), used=((S, K, M), u1), n_blacklist=((S,), i4),
                       blacklist_ids=((S, M), i4), n_order=((S,), i4), n_skipped=((S,), i4), skipped_pos=((S, M), i4),
                       skipped_id=((S, M), i4), cand_pos=((S, V), i4), cand_col=((S, V), i4)),
            session=dict(good_ring=((S, W), f4), ring_head=((S,), i4), ring_entries=((S,), i4), tracking_status=((S,), i4),
                         control_status=((S,), i4), last_reset_time=((S,), f8), first_sample=((S,), u1), first_sample_t=((S,), f8),
                         prev_sample_t=((S,), f8), time=((S,), f8), initialized_orientation=((S,), u1)),
            control=dict(zupt_time=((S,), f8), init_zupt_time=((S,), f8), was_stationary=((S,), i4), frames_since_keyframe=((S,), i4)),
            record=dict(t=((S,), f8), tracking_status=((S,), i4), stationary_visual=((S,), u1), inertial_mean=((S, 20), f8),
                        inertial_cov_diag=((S, 20), f8), position_cov=((S, 3, 3), f8), velocity_cov=((S, 3, 3), f8), n_trail=((S,), i4),
                        trail_time=((S, T), f8), trail_pose=((S, T, 7), f8), api_pose=((S, 7), f8), api_trail_pose=((S, T, 7), f8),
                        n_points=((S,), i4), point_id=((S, V), i4), point_status=((S, V), i4), point_first_pixel=((S, V, 2), f4),
                        point_xyz=((S, V, 3), f8)))
        rng = dict(mt=((S, RNG_STATE_WORDS), i4), pos=((S,), i4))
        out = {}
        for name, members in list(spec.items()) + [(k, rng) for k in ("rng_pipeline", "rng_ransac3", "rng_odometry")]:
            struct = getattr(raw, name)
            out[name] = {k: _wrap(getattr(struct, k), shape, ts) if getattr(struct, k) else None for k, (shape, ts) in members.items()}
        stage = dict(frame_num=((S,), i4), has_previous=((S,), u1), full_update=((S,), u1), keyframe=((S,), i4), keyframe_out=((S,), i4),
                     good_frame=((S,), u1), reset_kind=((S,), i4), tracking_status=((S,), i4), n_candidates=((S,), i4), cand_id=((V, S), i4),
                     status=((V, S, 2), i4), gate_status=((V, S), i4), slot_prev_left=((S,), i4), slot_cur_left=((S,), i4),
                     slot_right=((S,), i4), ransac_result=((S, 2), i4), ransac_score=((S,), f8), r5_summary=((S, 4), i4))
        for k, (shape, ts) in stage.items():
            out[k] = _wrap(getattr(raw, k), shape, ts) if getattr(raw, k) else None
        out["ekf_handle"] = C.c_void_p(raw.ekf)
        out["state_dim"] = lib().hv_ekf_state_dim(out["ekf_handle"])
        return out

    def state(self):
        """Means [n_sets][n] and covariances [n_sets][n][n] (column-major per filter) read back from the engine's filter."""
        raw = self.raw_view()
        h = C.c_void_p(raw.ekf)
        n = lib().hv_ekf_state_dim(h)
        ms, Ps = np.zeros((self.n_sets, n)), np.zeros((self.n_sets, n, n))
        for b in range(self.n_sets):
            self.ctx._chk(lib().hv_ekf_get_state(h, b, _p(ms[b], f64p), _p(Ps[b], f64p)), "hv_ekf_get_state")
        return ms, Ps
