"""include/orbhip.h restated once for Python: its structs as numpy dtypes / ctypes.Structures (RECORDS), its macros (MACROS) and its function
prototypes (PROTOTYPES); ORBD_PROTOTYPES does the same for include/orbd.h.  tests/test_abi.py compares all of it with the headers (a compiled
probe for sizes, offsets and macro values; the declarations for names and parameter counts), so a change there and a change here go together.
The modules that use a record re-export it under the name they always had (orbhip.matcher.QUERY_DTYPE, orbhip.lba.EDGE_DTYPE, ...)."""
import ctypes as C

import numpy as np

# ---- return codes --------------------------------------------------------------------------------------------------------------------
ORB_OK, ORB_E_EMPTY_IMAGE, ORB_E_CAPACITY, ORB_E_INVALID, ORB_E_HIP, ORB_E_NOMEM, ORB_E_ABORTED = 0, -1, -2, -3, -4, -5, -6

# ---- stage 1: ORBextractor ---------------------------------------------------------------------------------------------------------------
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])  # cv::KeyPoint, 28 B


class OrbxConfig(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32)]


# ---- stage 2: ORBmatcher ---------------------------------------------------------------------------------------------------------------
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30   # ORBmatcher.cc:36-38
GRID_COLS, GRID_ROWS = 64, 48                 # Frame.h:38-39
MODE_LOCAL_MAP, MODE_BEST_ONLY, MODE_INIT = 0, 1, 2
Q_VALID, Q_STEREO, Q_HAS_OBS, Q_RIGHT, Q_TWIN = 1, 2, 4, 8, 16

QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("u_right", "<f4"), ("angle", "<f4"),
                        ("min_level", "<i2"), ("max_level", "<i2"), ("flags", "<u4")])


class GridParams(C.Structure):
    _fields_ = [("min_x", C.c_float), ("min_y", C.c_float), ("grid_w_inv", C.c_float), ("grid_h_inv", C.c_float)]


class SearchParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("th_dist", C.c_int32), ("nn_ratio", C.c_float), ("check_orientation", C.c_int32),
                ("grid", GridParams)]


class BowSide(C.Structure):
    _fields_ = [("desc", C.c_void_p), ("angle", C.c_void_p), ("node_id", C.c_void_p), ("node_start", C.c_void_p),
                ("feat_idx", C.c_void_p), ("n_nodes", C.c_void_p), ("cap_f", C.c_int32), ("cap_nodes", C.c_int32), ("n_left", C.c_void_p)]


class FuseParams(C.Structure):
    _fields_ = [("th_dist", C.c_int32), ("chi2_gate", C.c_int32), ("grid", GridParams), ("inv_level_sigma2", C.c_float * 16)]


class TriSide(C.Structure):
    _fields_ = [("kps", C.c_void_p), ("desc", C.c_void_p), ("u_right", C.c_void_p), ("has_mp", C.c_void_p), ("node_id", C.c_void_p),
                ("node_start", C.c_void_p), ("feat_idx", C.c_void_p), ("n_nodes", C.c_void_p), ("cap_f", C.c_int32), ("cap_nodes", C.c_int32)]


TRI_PAIR_DTYPE = np.dtype([("F12", "<f4", (9,)), ("ep", "<f4", (2,)), ("level_sigma2_2", "<f4", (16,)), ("scale_factors_2", "<f4", (16,)),
                           ("reserved", "<f4")])
TRI_KB8_PAIR_DTYPE = np.dtype([("n_cams", "<i4"), ("reserved", "<i4"), ("k1", "<f4", (2, 8)), ("k2", "<f4", (2, 8)), ("R12", "<f4", (4, 9)),
                               ("t12", "<f4", (4, 3)), ("ep", "<f4", (2,)), ("level_sigma2_1", "<f4", (16,)), ("level_sigma2_2", "<f4", (16,)),
                               ("scale_factors_2", "<f4", (16,))])

# map-point projection records (include/orbhip.h "Map-point projection")
PROJ_LOCAL_MAP, PROJ_LAST_FRAME, PROJ_RELOC = 0, 1, 2
PROJ_CAM_PINHOLE = 0
MP_VALID, MP_BAD, MP_SEEN, MP_HAS_OBS = 1, 2, 4, 8
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"), ("angle", "<f4"),
                            ("octave", "<i4"), ("desc_row", "<i4"), ("flags", "<u4")])
TRACK_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("depth", "<f4"), ("view_cos", "<f4"), ("level", "<i4"),
                        ("in_view", "<i4"), ("reserved", "<i4")])
PROJECT_FRAME_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("Rlw", "<f4", (9,)), ("tlw", "<f4", (3,)),
                                ("bounds", "<f4", (4,))])


class ProjectParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("camera_type", C.c_int32), ("nleft", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("mbf", C.c_float), ("mb", C.c_float), ("mono", C.c_int32), ("th", C.c_float), ("view_cos_limit", C.c_float),
                ("far_points", C.c_int32), ("th_far_points", C.c_float), ("nlevels", C.c_int32), ("n_desc_rows", C.c_int32),
                ("scale_factors", C.c_float * 16), ("level_thresholds", C.c_float * 16)]


# map-point refresh records (include/orbhip.h "Map-point refresh")
OBS_RIGHT, OBS_KF_BAD = 1, 2
REFRESH_DESCRIPTOR, REFRESH_NORMAL_DEPTH = 1, 2
REFRESHED_DESCRIPTOR, REFRESHED_NORMAL_DEPTH, REFRESH_OVERFLOW, REFRESH_BAD_RECORD = 1, 2, 4, 8
REFRESH_MAX_OBS = 1024
OBSERVATION_DTYPE = np.dtype([("kf", "<i4"), ("desc_row", "<i4"), ("flags", "<u4")])
KEYFRAME_CENTER_DTYPE = np.dtype([("left", "<f4", (3,)), ("right", "<f4", (3,))])
REFRESH_POINT_DTYPE = np.dtype([("ref_kf", "<i4"), ("level", "<i4")])


class RefreshParams(C.Structure):
    _fields_ = [("what", C.c_uint32), ("nlevels", C.c_int32), ("scale_factors", C.c_float * 16)]


# Sim3Solver records (include/orbhip.h "Sim3Solver")
SIM3_CAM_PINHOLE, SIM3_CAM_KB8 = 0, 1
SIM3_BAD_SAMPLE, SIM3_ITS_CLAMPED, SIM3_N_CLAMPED, SIM3_BAD_INDEX = 1, 2, 4, 8
SIM3_MAX_N = 3392
SIM3_CAMERA_DTYPE = np.dtype([("model", "<i4"), ("p", "<f4", (8,))])
SIM3_CORR_DTYPE = np.dtype([("Xw1", "<f4", (3,)), ("Xw2", "<f4", (3,)), ("max_err1", "<f4"), ("max_err2", "<f4"), ("index1", "<i4")])
SIM3_PROBLEM_DTYPE = np.dtype([("Rcw1", "<f4", (9,)), ("tcw1", "<f4", (3,)), ("Rcw2", "<f4", (9,)), ("tcw2", "<f4", (3,)),
                               ("cam1", SIM3_CAMERA_DTYPE), ("cam2", SIM3_CAMERA_DTYPE), ("fix_scale", "<i4"), ("min_inliers", "<i4"),
                               ("max_its", "<i4"), ("n1", "<i4")])
SIM3_HYP_DTYPE = np.dtype([("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4")])
SIM3_RESULT_DTYPE = np.dtype([("iterations", "<i4"), ("converged", "<i4"), ("no_more", "<i4"), ("best_iter", "<i4"), ("n_inliers", "<i4"),
                              ("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4"), ("T12", "<f4", (16,)), ("status", "<u4")])

# TwoViewReconstruction records (include/orbhip.h "TwoViewReconstruction")
TVR_TOO_FEW, TVR_BAD_SAMPLE, TVR_BAD_INDEX, TVR_ITS_CLAMPED, TVR_N_CLAMPED, TVR_NAN_PARALLAX = 1, 2, 4, 8, 16, 32
TVR_PROBLEM_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("sigma", "<f4"), ("max_its", "<i4"), ("n_keys1", "<i4"),
                              ("n_keys2", "<i4"), ("min_parallax", "<f4"), ("min_triangulated", "<i4")])
TVR_RESULT_DTYPE = np.dtype([("R21", "<f4", (9,)), ("t21", "<f4", (3,)), ("SH", "<f4"), ("SF", "<f4"), ("best_it_H", "<i4"), ("best_it_F", "<i4"),
                             ("n_matches", "<i4"), ("n_inliers", "<i4"), ("model", "<i4"), ("hypothesis", "<i4"), ("n_good", "<i4"),
                             ("parallax", "<f4"), ("ok", "<i4"), ("status", "<u4")])

# new map points (include/orbhip.h "New map points")
NEWPT_CAM_PINHOLE, NEWPT_CAM_KB8 = PROJ_CAM_PINHOLE, 1
(NEWPT_NO_MATCH, NEWPT_CREATED_TRIANGULATED, NEWPT_CREATED_STEREO1, NEWPT_CREATED_STEREO2, NEWPT_LOW_PARALLAX, NEWPT_W_ZERO, NEWPT_EMPTY_STEREO,
 NEWPT_BEHIND_1, NEWPT_BEHIND_2, NEWPT_REPROJ_1, NEWPT_REPROJ_2, NEWPT_ZERO_DIST, NEWPT_FAR, NEWPT_SCALE, NEWPT_BAD_INDEX) = range(15)
NEWPT_PAIR_BAD_INDEX, NEWPT_PAIR_OVERFLOW, NEWPT_PAIR_BAD_CAMERA = 1, 2, 4
NEWPT_CAMERA_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("camera_type", "<i4"), ("k", "<f4", (8,)),
                               ("invfx", "<f4"), ("invfy", "<f4"), ("mb", "<f4"), ("mbf", "<f4"), ("level_sigma2", "<f4", (16,)),
                               ("scale_factors", "<f4", (16,))])
NEWPT_PAIR_DTYPE = np.dtype([("cam1", NEWPT_CAMERA_DTYPE), ("cam2", NEWPT_CAMERA_DTYPE), ("ratio_factor", "<f4"), ("far_points", "<i4"),
                             ("th_far_points", "<f4"), ("kf1", "<i4"), ("kf2", "<i4"), ("obs_kf2_first", "<i4"), ("desc_row0_1", "<i4"),
                             ("desc_row0_2", "<i4")])
NEW_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("idx1", "<i4"), ("idx2", "<i4"), ("how", "<i4")])


class NewPtSide(C.Structure):
    _fields_ = [("kps", C.c_void_p), ("kps_raw", C.c_void_p), ("u_right", C.c_void_p), ("depth", C.c_void_p), ("n", C.c_void_p),
                ("has_mp", C.c_void_p), ("cap_f", C.c_int32), ("reserved", C.c_int32)]


# local map (include/orbhip.h "Local map")
LM_KF_PRESENT, LM_KF_BAD = 1, 2
LM_INERTIAL = 1
LM_KF_OVERFLOW, LM_MP_OVERFLOW, LM_BAD_INDEX = 1, 2, 4
LOCALMAP_KEYFRAME_DTYPE = np.dtype([("flags", "<u4"), ("parent", "<i4"), ("prev", "<i4"), ("mp_row0", "<i4"), ("n_feat", "<i4"),
                                    ("covis", "<i4", (10,)), ("child_start", "<i4"), ("n_child", "<i4"), ("reserved", "<i4")])
LOCALMAP_FRAME_DTYPE = np.dtype([("last_kf", "<i4"), ("flags", "<u4")])


class LocalMapView(C.Structure):
    _fields_ = [("d_mp", C.c_void_p), ("d_obs_start", C.c_void_p), ("d_obs", C.c_void_p), ("d_kf", C.c_void_p), ("d_kf_mp", C.c_void_p),
                ("d_children", C.c_void_p), ("d_kf_by_order", C.c_void_p), ("d_mp_track", C.c_void_p), ("n_mp", C.c_int32),
                ("n_obs", C.c_int32), ("n_kf", C.c_int32), ("n_kf_mp_rows", C.c_int32), ("n_children", C.c_int32), ("track_stride", C.c_int32)]


class LocalMapLists(C.Structure):
    _fields_ = [("d_vote_mp", C.c_void_p), ("d_n_vote", C.c_void_p), ("d_frame_mp", C.c_void_p), ("d_n_frame", C.c_void_p),
                ("d_dropped_mp", C.c_void_p), ("d_n_dropped", C.c_void_p), ("cap_f", C.c_int32), ("cap_dropped", C.c_int32)]


class LocalMapOut(C.Structure):
    _fields_ = [("d_local_kf", C.c_void_p), ("d_n_local_kf", C.c_void_p), ("d_n_local_kf_required", C.c_void_p), ("d_ref_kf", C.c_void_p),
                ("d_max_votes", C.c_void_p), ("d_local_src", C.c_void_p), ("d_nmp", C.c_void_p), ("d_nmp_required", C.c_void_p),
                ("d_local_mp", C.c_void_p), ("d_track", C.c_void_p), ("d_flags", C.c_void_p), ("cap_kf", C.c_int32), ("cap_mp", C.c_int32)]


# key-frame culling (include/orbhip.h "Key-frame culling")
CULL_KF_NOT_ERASE = 1
CULL_FEAT_OCTAVE, CULL_FEAT_CLOSE, CULL_FEAT_STEREO = 0x3F, 0x40, 0x80
CULL_INERTIAL, CULL_MONOCULAR, CULL_IMU_INITIALIZED, CULL_INERTIAL_BA2, CULL_ABORT_BA = 1, 2, 4, 8, 16
(CULL_CODE_NOT_VISITED, CULL_CODE_SKIPPED, CULL_CODE_KEPT, CULL_CODE_KEPT_FEW_KFS, CULL_CODE_KEPT_RECENT, CULL_CODE_KEPT_NO_NEIGHBOUR,
 CULL_CODE_KEPT_INERTIAL, CULL_CODE_CULLED, CULL_CODE_CULLED_IMU1, CULL_CODE_CULLED_IMU2) = range(10)
CULL_CODE_DEFERRED = 0x80
CULL_BAD_INDEX, CULL_UNSUPPORTED = 1, 2
CULL_REC_LIVE, CULL_REC_ERASED_BY_KF, CULL_REC_ERASED_BY_POINT, CULL_REC_ABSENT = 0, 1, 2, 3
CULL_KEYFRAME_DTYPE = np.dtype([("timestamp", "<f8"), ("id", "<u4"), ("prev", "<i4"), ("next", "<i4"), ("desc_row0", "<i4"),
                                ("imu_pos", "<f4", (3,)), ("flags", "<u4")])
CULL_PROBLEM_DTYPE = np.dtype([("current_kf", "<i4"), ("init_kf_id", "<u4"), ("cand_start", "<i4"), ("n_cand", "<i4"), ("n_kf_in_map", "<i4"),
                               ("flags", "<u4")])
CULL_EVENT_DTYPE = np.dtype([("kf", "<i4"), ("prev", "<i4"), ("next", "<i4")])


class CullIn(C.Structure):
    _fields_ = [("d_ckf", C.c_void_p), ("d_feat", C.c_void_p), ("d_mp_nobs", C.c_void_p), ("d_problems", C.c_void_p),
                ("d_candidates", C.c_void_p), ("n_candidates", C.c_int32), ("n_cand_max", C.c_int32)]


class CullOut(C.Structure):
    _fields_ = [("d_code", C.c_void_p), ("d_nmps", C.c_void_p), ("d_nred", C.c_void_p), ("d_events", C.c_void_p), ("d_n_events", C.c_void_p),
                ("d_flags", C.c_void_p), ("cap_cand", C.c_int32), ("reserved", C.c_int32)]


class CullWorkspaceLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in ("stride", "nobs", "rec", "prev", "next", "mp_bad", "kf_erased")]


class CullApply(C.Structure):
    _fields_ = [("d_mp", C.c_void_p), ("d_kf", C.c_void_p), ("d_ckf", C.c_void_p), ("d_kf_mp", C.c_void_p), ("d_mp_nobs", C.c_void_p),
                ("d_ref", C.c_void_p), ("d_obs_start_out", C.c_void_p), ("d_obs_out", C.c_void_p), ("d_result", C.c_void_p),
                ("cap_obs_out", C.c_int32), ("reserved", C.c_int32)]


# covisibility graph (include/orbhip.h "Covisibility graph")
COVIS_KF_FIRST_CONNECTION = 1
COVIS_BAD_INDEX, COVIS_OVERFLOW = 1, 2
COVIS_ENTRY_DTYPE = np.dtype([("kf", "<i4"), ("weight", "<i4")])
COVIS_KEYFRAME_DTYPE = np.dtype([("id", "<u4"), ("map_id", "<i4"), ("flags", "<u4"), ("reserved", "<i4")])
COVIS_CHILD_EVENT_DTYPE = np.dtype([("child", "<i4"), ("parent", "<i4")])


class CovisStore(C.Structure):
    _fields_ = [("d_conn", C.c_void_p), ("d_n_conn", C.c_void_p), ("d_ordered_kf", C.c_void_p), ("d_ordered_w", C.c_void_p),
                ("d_n_ordered", C.c_void_p), ("cap_conn", C.c_int32), ("reserved", C.c_int32)]


class CovisOut(C.Structure):
    _fields_ = [("d_child_events", C.c_void_p), ("d_n_child_events", C.c_void_p), ("d_nmax", C.c_void_p), ("d_kfmax", C.c_void_p),
                ("d_n_counter", C.c_void_p), ("d_overflow_kf", C.c_void_p), ("d_flags", C.c_void_p)]


# fusion in the neighbours (include/orbhip.h "Fusion in the neighbours")
FUSENB_MONOCULAR, FUSENB_INERTIAL, FUSENB_ABORT_BA = 1, 2, 4
FUSENB_MAX_TARGETS = 420
(FUSENB_EV_ADD, FUSENB_EV_LIST_POINT_REPLACED, FUSENB_EV_KF_POINT_REPLACED, FUSENB_EV_NOOP_BAD, FUSENB_EV_NOOP_SAME) = range(5)
(FUSENB_R_FLAGS, FUSENB_R_N_TARGETS, FUSENB_R_N_TARGETS_REQUIRED, FUSENB_R_N_CANDIDATES, FUSENB_R_N_CANDIDATES_REQUIRED, FUSENB_R_N_EVENTS,
 FUSENB_R_N_OBS, FUSENB_R_N_SEL, FUSENB_R_WORDS) = range(9)
(FUSENB_BAD_INDEX, FUSENB_UNSUPPORTED, FUSENB_TARGET_OVERFLOW, FUSENB_CANDIDATE_OVERFLOW, FUSENB_EVENT_OVERFLOW, FUSENB_OBS_OVERFLOW,
 FUSENB_REFRESH_OVERFLOW, FUSENB_UNSORTED) = (1 << i for i in range(8))
FUSENB_POSE_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("reserved", "<i4")])
FUSENB_EVENT_DTYPE = np.dtype([("call", "<i4"), ("kf", "<i4"), ("list_index", "<i4"), ("point", "<i4"), ("feature", "<i4"), ("other", "<i4"),
                               ("kind", "<i4"), ("reserved", "<i4")])


class FuseNbParams(C.Structure):
    _fields_ = [("current_kf", C.c_int32), ("flags", C.c_uint32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("mbf", C.c_float), ("th", C.c_float), ("bounds", C.c_float * 4), ("grid", GridParams), ("nlevels", C.c_int32),
                ("reserved", C.c_int32), ("scale_factors", C.c_float * 16), ("inv_level_sigma2", C.c_float * 16),
                ("level_thresholds", C.c_float * 16)]


class FuseNbIn(C.Structure):
    _fields_ = [("d_ckf", C.c_void_p), ("d_pose", C.c_void_p), ("d_feat", C.c_void_p), ("d_kps", C.c_void_p), ("d_u_right", C.c_void_p),
                ("d_kf_desc", C.c_void_p), ("d_ordered_kf", C.c_void_p), ("d_n_ordered", C.c_void_p), ("d_mp_nobs", C.c_void_p),
                ("n_kf_desc_rows", C.c_int32), ("cap_conn", C.c_int32), ("cap_feat", C.c_int32), ("reserved", C.c_int32)]


class FuseNbOut(C.Structure):
    _fields_ = [("d_mp", C.c_void_p), ("d_kf_mp", C.c_void_p), ("d_mp_nobs", C.c_void_p), ("d_found", C.c_void_p), ("d_visible", C.c_void_p),
                ("d_mp_desc", C.c_void_p), ("d_fuse_target", C.c_void_p), ("d_targets", C.c_void_p), ("d_candidates", C.c_void_p),
                ("d_nfused", C.c_void_p), ("d_events", C.c_void_p), ("d_replaced", C.c_void_p), ("d_sel", C.c_void_p),
                ("d_obs_start_out", C.c_void_p), ("d_obs_out", C.c_void_p), ("d_result", C.c_void_p), ("n_desc_rows", C.c_int32),
                ("cap_targets", C.c_int32), ("cap_candidates", C.c_int32), ("cap_events", C.c_int32), ("cap_obs_out", C.c_int32),
                ("reserved", C.c_int32)]


# new key frame (include/orbhip.h "New key frame")
(NEWKF_CODE_NOT_VISITED, NEWKF_CODE_NONE, NEWKF_CODE_BAD_POINT, NEWKF_CODE_ADDED, NEWKF_CODE_PUSHED, NEWKF_CODE_PUSHED_DUP,
 NEWKF_CODE_BAD_INDEX) = range(7)
NEWKF_R_FLAGS, NEWKF_R_N_ADDED, NEWKF_R_N_PUSHED, NEWKF_R_N_PUSH_REQUIRED, NEWKF_R_N_OBS, NEWKF_R_WORDS = 0, 1, 2, 3, 4, 8
(NEWKF_BAD_INDEX, NEWKF_UNSUPPORTED, NEWKF_OBS_OVERFLOW, NEWKF_RECENT_OVERFLOW, NEWKF_REFRESH_OVERFLOW, NEWKF_UNSORTED) = (1 << i for i in range(6))
MPCULL_MONOCULAR = 1
(MPCULL_CODE_NOT_VISITED, MPCULL_CODE_ERASED_BAD, MPCULL_CODE_CULLED_RATIO, MPCULL_CODE_CULLED_OBS, MPCULL_CODE_RETIRED, MPCULL_CODE_KEPT,
 MPCULL_CODE_BAD_INDEX) = range(7)


class NewKfIn(C.Structure):
    _fields_ = [("d_ckf", C.c_void_p), ("d_feat", C.c_void_p), ("d_ref", C.c_void_p), ("d_center", C.c_void_p), ("d_kf_desc", C.c_void_p),
                ("d_found", C.c_void_p), ("d_visible", C.c_void_p), ("d_first_kf_id", C.c_void_p), ("n_kf_desc_rows", C.c_int32),
                ("cap_feat", C.c_int32)]


class NewKfOut(C.Structure):
    _fields_ = [("d_mp", C.c_void_p), ("d_mp_nobs", C.c_void_p), ("d_mp_desc", C.c_void_p), ("d_code", C.c_void_p), ("d_sel", C.c_void_p),
                ("d_obs_start_out", C.c_void_p), ("d_obs_out", C.c_void_p), ("d_recent", C.c_void_p), ("d_n_recent", C.c_void_p),
                ("d_result", C.c_void_p), ("n_desc_rows", C.c_int32), ("cap_obs_out", C.c_int32), ("cap_recent", C.c_int32),
                ("reserved", C.c_int32)]


class MpCullOut(C.Structure):
    _fields_ = [("d_mp", C.c_void_p), ("d_kf_mp", C.c_void_p), ("d_code", C.c_void_p), ("d_recent_out", C.c_void_p),
                ("d_n_recent_out", C.c_void_p), ("d_culled", C.c_void_p), ("d_n_culled", C.c_void_p), ("d_obs_start_out", C.c_void_p),
                ("d_obs_out", C.c_void_p), ("d_result", C.c_void_p), ("cap_obs_out", C.c_int32), ("cap_recent", C.c_int32)]


# local bundle adjustment on the device map (include/orbhip.h "Local bundle adjustment on the device map")
(LBA_R_FLAGS, LBA_R_N_LOCAL, LBA_R_N_FIXED, LBA_R_NUM_FIXED_KF, LBA_R_N_POINTS, LBA_R_N_EDGES, LBA_R_N_MONO, LBA_R_N_STEREO,
 LBA_R_N_POSES_REQUIRED, LBA_R_N_POINTS_REQUIRED, LBA_R_N_EDGES_REQUIRED) = range(11)
LBA_R_WORDS = 12
LBA_BAD_INDEX, LBA_UNSUPPORTED, LBA_OVERFLOW, LBA_EARLY_RETURN = 1, 2, 4, 8
LBA_A_FLAGS, LBA_A_N_ERASED, LBA_A_N_WENT_BAD, LBA_A_N_OBS, LBA_A_N_MONO, LBA_A_N_STEREO, LBA_A_WORDS = 0, 1, 2, 3, 4, 5, 8


class LbaIn(C.Structure):
    _fields_ = [("d_ckf", C.c_void_p), ("d_pose", C.c_void_p), ("d_kps", C.c_void_p), ("d_u_right", C.c_void_p), ("d_ordered_kf", C.c_void_p),
                ("d_n_ordered", C.c_void_p), ("d_map", C.c_void_p), ("cap_conn", C.c_int32), ("nlevels", C.c_int32),
                ("inv_level_sigma2", C.c_float * 16), ("scale_factors", C.c_float * 16)]


class LbaWindow(C.Structure):
    _fields_ = [("poses", C.c_void_p), ("pose_hidx", C.c_void_p), ("points", C.c_void_p), ("edges", C.c_void_p), ("lm_start", C.c_void_p),
                ("pose_start", C.c_void_p), ("pose_edges", C.c_void_p), ("n_poses", C.c_void_p), ("n_points", C.c_void_p),
                ("n_edges", C.c_void_p), ("d_pose_kf", C.c_void_p), ("d_pose_local", C.c_void_p), ("d_point_mp", C.c_void_p),
                ("d_edge_rec", C.c_void_p), ("d_result", C.c_void_p), ("cap_p", C.c_int32), ("cap_l", C.c_int32), ("cap_e", C.c_int32),
                ("reserved", C.c_int32)]


class LbaApply(C.Structure):
    _fields_ = [("d_mp", C.c_void_p), ("d_kf_mp", C.c_void_p), ("d_mp_nobs", C.c_void_p), ("d_ref", C.c_void_p), ("d_pose", C.c_void_p),
                ("d_center", C.c_void_p), ("d_erased", C.c_void_p), ("d_went_bad", C.c_void_p), ("d_obs_start_out", C.c_void_p),
                ("d_obs_out", C.c_void_p), ("d_result", C.c_void_p), ("cap_obs_out", C.c_int32), ("reserved", C.c_int32)]


# ---- Frame constructor steps ---------------------------------------------------------------------------------------------------------------
class Camera(C.Structure):
    """Pinhole::toK() + mDistCoef (k1, k2, p1, p2, k3)"""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("dist", C.c_float * 5)]

    @classmethod
    def make(cls, fx, fy, cx, cy, dist=()):
        d = list(dist) + [0.0] * (5 - len(dist))
        return cls(fx, fy, cx, cy, (C.c_float * 5)(*d))

    def as_array(self):
        return np.array([self.fx, self.fy, self.cx, self.cy] + list(self.dist), np.float32)


class FisheyeRig(C.Structure):
    """KannalaBrandt8 parameters of mpCamera / mpCamera2, mRlr / mtlr (Frame.cc:1242-1243), mvLevelSigma2"""
    _fields_ = [("k_left", C.c_float * 8), ("k_right", C.c_float * 8), ("R_lr", C.c_float * 9), ("t_lr", C.c_float * 3), ("level_sigma2", C.c_float * 16)]

    @classmethod
    def make(cls, k_left, k_right, R_lr, t_lr, level_sigma2):
        ls = list(level_sigma2) + [0.0] * (16 - len(level_sigma2))
        return cls((C.c_float * 8)(*[float(v) for v in k_left]), (C.c_float * 8)(*[float(v) for v in k_right]),
                   (C.c_float * 9)(*[float(v) for v in np.asarray(R_lr).reshape(-1)]), (C.c_float * 3)(*[float(v) for v in t_lr]), (C.c_float * 16)(*ls))

    def as_array(self):
        return np.array(list(self.k_left) + list(self.k_right) + list(self.R_lr) + list(self.t_lr), np.float32)


# ---- DBoW2 transform and place recognition ---------------------------------------------------------------------------------------------------
class BowResult(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("word_id", "node_id", "weight", "fv_node_id", "fv_node_start", "fv_feat_idx", "fv_n_nodes", "bv_word",
                                          "bv_value", "bv_n")]


KF_PRESENT, COVIS, MAX_CANDIDATES, BOWDB_L1_NORM = 1, 10, 64, 0
KEYFRAME_DTYPE = np.dtype([("flags", "<u4"), ("map_id", "<i4"), ("seq", "<u4"), ("covis", "<i4", (COVIS,))])
BOWDB_QUERY_DTYPE = np.dtype([("id", "<u8"), ("map_id", "<i4"), ("row", "<i4"), ("conn_start", "<i4"), ("conn_n", "<i4")])
STATS_DTYPE = np.dtype([("n_sharing", "<i4"), ("max_common_words", "<i4"), ("n_scored", "<i4"), ("best_acc_score", "<f4")])


class View(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("bv_word", "bv_value", "bv_n", "kf", "reloc_query", "reloc_score", "place_query", "place_score",
                                          "map_bad")] + [(n, C.c_int32) for n in ("n_slots", "cap_f", "n_maps", "scoring")]


class QueryBows(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("q_word", "q_value", "q_n")] + [("n_rows", C.c_int32), ("cap_q", C.c_int32)]


# ---- stage 3: bundle adjustment, pose optimisation, inertial windows ---------------------------------------------------------------------------
EDGE_MONO, EDGE_STEREO, EDGE_BODY = 0, 1, 2
CAM_PINHOLE, CAM_KB8 = 0, 1
HINT_MONO_PINHOLE, HINT_PINHOLE = 1, 2
EDGE_DTYPE = np.dtype([("pose", "<i4"), ("point", "<i4"), ("kind", "<i2"), ("cam", "<i2"), ("obs", "<f4", (3,)), ("inv_sigma2", "<f4")])
CAM_DTYPE = np.dtype([("model", "<i4"), ("reserved", "<i4"), ("p", "<f8", (8,)), ("bf", "<f8"), ("trl_q", "<f8", (4,)), ("trl_t", "<f8", (3,))])
POSE_EDGE_DTYPE = np.dtype([("xw", "<f4", (3,)), ("obs", "<f4", (3,)), ("inv_sigma2", "<f4"), ("kind", "<i2"), ("cam", "<i2")])


class LbaProblem(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("poses", "pose_hidx", "points", "edges", "lm_start", "pose_start", "pose_edges", "cameras",
                                          "n_poses", "n_points", "n_edges")] + \
               [("cap_p", C.c_int32), ("cap_l", C.c_int32), ("cap_e", C.c_int32), ("n_cameras", C.c_int32),
                ("huber_mono", C.c_double), ("huber_stereo", C.c_double)]


class LbaSystem(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("Hpp", "bp", "Hll", "bl", "Hpl", "err", "chi2", "rho", "depth", "robust_chi2_sum")]


LBA_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)   # lba_allreduce_fn

KF_DTYPE = np.dtype([("Rwb", "<f8", (9,)), ("twb", "<f8", (3,)), ("Rcw", "<f8", (2, 9)), ("tcw", "<f8", (2, 3)), ("v", "<f8", (3,)),
                     ("bg", "<f8", (3,)), ("ba", "<f8", (3,)), ("pose_fixed", "<i4"), ("has_imu", "<i4"), ("imu_fixed", "<i4"), ("reserved", "<i4")])
IMU_EDGE_DTYPE = np.dtype([("kf1", "<i4"), ("kf2", "<i4"), ("dR", "<f4", (9,)), ("dV", "<f4", (3,)), ("dP", "<f4", (3,)), ("JRg", "<f4", (9,)),
                           ("JVg", "<f4", (9,)), ("JVa", "<f4", (9,)), ("JPg", "<f4", (9,)), ("JPa", "<f4", (9,)), ("b", "<f4", (6,)), ("dT", "<f4"),
                           ("pad", "<f4"), ("huber", "<f8"), ("info", "<f8", (81,)), ("info_g", "<f8", (9,)), ("info_a", "<f8", (9,))])
PRIOR_DTYPE = np.dtype([("Rwb", "<f8", (9,)), ("twb", "<f8", (3,)), ("vwb", "<f8", (3,)), ("bg", "<f8", (3,)), ("ba", "<f8", (3,)), ("H", "<f8", (225,))])
LIBA_MAX_FREE = 32
EDGE_CLOSE = 0x100   # pose_edge.kind flag: pFrame->mvpMapPoints[idx]->mTrackDepth < 10.f (Optimizer.cc:7852)


class Rig(C.Structure):
    """Calibration members of ImuCamPose (G2oTypes.h:60-72): per camera Rcb, tcb, Rbc, tbc; bf; camera model + parameters."""
    _fields_ = [("n_cams", C.c_int32), ("reserved", C.c_int32), ("Rcb", (C.c_double * 9) * 2), ("tcb", (C.c_double * 3) * 2),
                ("Rbc", (C.c_double * 9) * 2), ("tbc", (C.c_double * 3) * 2), ("bf", C.c_double), ("model", C.c_int32 * 2), ("p", (C.c_double * 8) * 2)]


class LibaProblem(C.Structure):
    _fields_ = [("kfs", C.c_void_p), ("n_kf", C.c_void_p), ("rigs", C.c_void_p), ("points", C.c_void_p), ("n_points", C.c_void_p),
                ("edges", C.c_void_p), ("n_edges", C.c_void_p), ("imu", C.c_void_p), ("n_imu", C.c_void_p),
                ("cap_kf", C.c_int32), ("cap_l", C.c_int32), ("cap_e", C.c_int32), ("cap_i", C.c_int32), ("rig_stride", C.c_int32),
                ("max_free", C.c_int32), ("huber_mono", C.c_double), ("huber_stereo", C.c_double)]


# ---- the tables tests/test_abi.py checks against the headers ---------------------------------------------------------------------------------
RECORDS = {
    "orb_keypoint": KP_DTYPE, "orbx_config": OrbxConfig, "orbm_grid_params": GridParams, "orbf_camera": Camera, "orbf_fisheye_rig": FisheyeRig,
    "orbm_query": QUERY_DTYPE, "orbm_search_params": SearchParams, "orbm_map_point": MAP_POINT_DTYPE, "orbm_track": TRACK_DTYPE,
    "orbm_project_frame": PROJECT_FRAME_DTYPE, "orbm_project_params": ProjectParams, "orbm_observation": OBSERVATION_DTYPE,
    "orbm_keyframe_center": KEYFRAME_CENTER_DTYPE, "orbm_refresh_point": REFRESH_POINT_DTYPE, "orbm_refresh_params": RefreshParams,
    "orbm_sim3_camera": SIM3_CAMERA_DTYPE, "orbm_sim3_corr": SIM3_CORR_DTYPE, "orbm_sim3_problem": SIM3_PROBLEM_DTYPE,
    "orbm_sim3_hyp": SIM3_HYP_DTYPE, "orbm_sim3_result": SIM3_RESULT_DTYPE,
    "orbm_tvr_problem": TVR_PROBLEM_DTYPE, "orbm_tvr_result": TVR_RESULT_DTYPE,
    "orbm_newpt_camera": NEWPT_CAMERA_DTYPE, "orbm_newpt_pair": NEWPT_PAIR_DTYPE, "orbm_newpt_side": NewPtSide, "orbm_new_point": NEW_POINT_DTYPE,
    "orbm_localmap_keyframe": LOCALMAP_KEYFRAME_DTYPE, "orbm_localmap_view": LocalMapView, "orbm_localmap_frame": LOCALMAP_FRAME_DTYPE,
    "orbm_localmap_lists": LocalMapLists, "orbm_localmap_out": LocalMapOut,
    "orbm_cull_keyframe": CULL_KEYFRAME_DTYPE, "orbm_cull_problem": CULL_PROBLEM_DTYPE, "orbm_cull_in": CullIn, "orbm_cull_event": CULL_EVENT_DTYPE,
    "orbm_cull_out": CullOut, "orbm_cull_workspace_layout": CullWorkspaceLayout, "orbm_cull_apply": CullApply,
    "orbm_covis_entry": COVIS_ENTRY_DTYPE, "orbm_covis_keyframe": COVIS_KEYFRAME_DTYPE, "orbm_covis_store": CovisStore,
    "orbm_covis_child_event": COVIS_CHILD_EVENT_DTYPE, "orbm_covis_out": CovisOut,
    "orbm_fusenb_pose": FUSENB_POSE_DTYPE, "orbm_fusenb_params": FuseNbParams, "orbm_fusenb_in": FuseNbIn,
    "orbm_fusenb_event": FUSENB_EVENT_DTYPE, "orbm_fusenb_out": FuseNbOut,
    "orbm_newkf_in": NewKfIn, "orbm_newkf_out": NewKfOut, "orbm_mpcull_out": MpCullOut,
    "orbm_lba_in": LbaIn, "orbm_lba_window": LbaWindow, "orbm_lba_apply": LbaApply,
    "orbm_fuse_params": FuseParams, "orbm_tri_side": TriSide, "orbm_tri_pair": TRI_PAIR_DTYPE, "orbm_tri_kb8_pair": TRI_KB8_PAIR_DTYPE,
    "orbm_bow_side": BowSide, "bow_result": BowResult, "bowdb_keyframe": KEYFRAME_DTYPE, "bowdb_view": View, "bowdb_query": BOWDB_QUERY_DTYPE,
    "bowdb_query_bows": QueryBows, "bowdb_stats": STATS_DTYPE, "lba_camera": CAM_DTYPE, "lba_edge": EDGE_DTYPE, "lba_problem": LbaProblem,
    "lba_system": LbaSystem, "pose_edge": POSE_EDGE_DTYPE, "liba_keyframe": KF_DTYPE, "liba_rig": Rig, "liba_imu_edge": IMU_EDGE_DTYPE,
    "liba_problem": LibaProblem, "liba_prior": PRIOR_DTYPE,
}

MACROS = {
    "ORB_OK": ORB_OK, "ORB_E_EMPTY_IMAGE": ORB_E_EMPTY_IMAGE, "ORB_E_CAPACITY": ORB_E_CAPACITY, "ORB_E_INVALID": ORB_E_INVALID,
    "ORB_E_HIP": ORB_E_HIP, "ORB_E_NOMEM": ORB_E_NOMEM, "ORB_E_ABORTED": ORB_E_ABORTED,
    "ORBM_TH_HIGH": TH_HIGH, "ORBM_TH_LOW": TH_LOW, "ORBM_HISTO_LENGTH": HISTO_LENGTH, "ORBM_GRID_COLS": GRID_COLS, "ORBM_GRID_ROWS": GRID_ROWS,
    "ORBM_Q_VALID": Q_VALID, "ORBM_Q_STEREO": Q_STEREO, "ORBM_Q_HAS_OBS": Q_HAS_OBS, "ORBM_Q_RIGHT": Q_RIGHT, "ORBM_Q_TWIN": Q_TWIN,
    "ORBM_MODE_LOCAL_MAP": MODE_LOCAL_MAP, "ORBM_MODE_BEST_ONLY": MODE_BEST_ONLY, "ORBM_MODE_INIT": MODE_INIT,
    "ORBM_MP_VALID": MP_VALID, "ORBM_MP_BAD": MP_BAD, "ORBM_MP_SEEN": MP_SEEN, "ORBM_MP_HAS_OBS": MP_HAS_OBS,
    "ORBM_PROJ_LOCAL_MAP": PROJ_LOCAL_MAP, "ORBM_PROJ_LAST_FRAME": PROJ_LAST_FRAME, "ORBM_PROJ_RELOC": PROJ_RELOC,
    "ORBM_CAM_PINHOLE": PROJ_CAM_PINHOLE,
    "ORBM_OBS_RIGHT": OBS_RIGHT, "ORBM_OBS_KF_BAD": OBS_KF_BAD,
    "ORBM_REFRESH_DESCRIPTOR": REFRESH_DESCRIPTOR, "ORBM_REFRESH_NORMAL_DEPTH": REFRESH_NORMAL_DEPTH,
    "ORBM_REFRESHED_DESCRIPTOR": REFRESHED_DESCRIPTOR, "ORBM_REFRESHED_NORMAL_DEPTH": REFRESHED_NORMAL_DEPTH,
    "ORBM_REFRESH_OVERFLOW": REFRESH_OVERFLOW, "ORBM_REFRESH_BAD_RECORD": REFRESH_BAD_RECORD, "ORBM_REFRESH_MAX_OBS": REFRESH_MAX_OBS,
    "ORBM_SIM3_CAM_PINHOLE": SIM3_CAM_PINHOLE, "ORBM_SIM3_CAM_KB8": SIM3_CAM_KB8, "ORBM_SIM3_BAD_SAMPLE": SIM3_BAD_SAMPLE,
    "ORBM_SIM3_ITS_CLAMPED": SIM3_ITS_CLAMPED, "ORBM_SIM3_N_CLAMPED": SIM3_N_CLAMPED, "ORBM_SIM3_BAD_INDEX": SIM3_BAD_INDEX,
    "ORBM_SIM3_MAX_N": SIM3_MAX_N,
    "ORBM_TVR_TOO_FEW": TVR_TOO_FEW, "ORBM_TVR_BAD_SAMPLE": TVR_BAD_SAMPLE, "ORBM_TVR_BAD_INDEX": TVR_BAD_INDEX,
    "ORBM_TVR_ITS_CLAMPED": TVR_ITS_CLAMPED, "ORBM_TVR_N_CLAMPED": TVR_N_CLAMPED, "ORBM_TVR_NAN_PARALLAX": TVR_NAN_PARALLAX,
    "ORBM_CAM_KB8": NEWPT_CAM_KB8, "ORBM_NEWPT_NO_MATCH": NEWPT_NO_MATCH, "ORBM_NEWPT_CREATED_TRIANGULATED": NEWPT_CREATED_TRIANGULATED,
    "ORBM_NEWPT_CREATED_STEREO1": NEWPT_CREATED_STEREO1, "ORBM_NEWPT_CREATED_STEREO2": NEWPT_CREATED_STEREO2,
    "ORBM_NEWPT_LOW_PARALLAX": NEWPT_LOW_PARALLAX, "ORBM_NEWPT_W_ZERO": NEWPT_W_ZERO, "ORBM_NEWPT_EMPTY_STEREO": NEWPT_EMPTY_STEREO,
    "ORBM_NEWPT_BEHIND_1": NEWPT_BEHIND_1, "ORBM_NEWPT_BEHIND_2": NEWPT_BEHIND_2, "ORBM_NEWPT_REPROJ_1": NEWPT_REPROJ_1,
    "ORBM_NEWPT_REPROJ_2": NEWPT_REPROJ_2, "ORBM_NEWPT_ZERO_DIST": NEWPT_ZERO_DIST, "ORBM_NEWPT_FAR": NEWPT_FAR, "ORBM_NEWPT_SCALE": NEWPT_SCALE,
    "ORBM_NEWPT_BAD_INDEX": NEWPT_BAD_INDEX, "ORBM_NEWPT_PAIR_BAD_INDEX": NEWPT_PAIR_BAD_INDEX, "ORBM_NEWPT_PAIR_OVERFLOW": NEWPT_PAIR_OVERFLOW,
    "ORBM_NEWPT_PAIR_BAD_CAMERA": NEWPT_PAIR_BAD_CAMERA,
    "ORBM_LM_KF_PRESENT": LM_KF_PRESENT, "ORBM_LM_KF_BAD": LM_KF_BAD, "ORBM_LM_INERTIAL": LM_INERTIAL, "ORBM_LM_KF_OVERFLOW": LM_KF_OVERFLOW,
    "ORBM_LM_MP_OVERFLOW": LM_MP_OVERFLOW, "ORBM_LM_BAD_INDEX": LM_BAD_INDEX,
    "ORBM_CULL_KF_NOT_ERASE": CULL_KF_NOT_ERASE, "ORBM_CULL_FEAT_OCTAVE": CULL_FEAT_OCTAVE, "ORBM_CULL_FEAT_CLOSE": CULL_FEAT_CLOSE,
    "ORBM_CULL_FEAT_STEREO": CULL_FEAT_STEREO, "ORBM_CULL_INERTIAL": CULL_INERTIAL, "ORBM_CULL_MONOCULAR": CULL_MONOCULAR,
    "ORBM_CULL_IMU_INITIALIZED": CULL_IMU_INITIALIZED, "ORBM_CULL_INERTIAL_BA2": CULL_INERTIAL_BA2, "ORBM_CULL_ABORT_BA": CULL_ABORT_BA,
    "ORBM_CULL_CODE_NOT_VISITED": CULL_CODE_NOT_VISITED, "ORBM_CULL_CODE_SKIPPED": CULL_CODE_SKIPPED, "ORBM_CULL_CODE_KEPT": CULL_CODE_KEPT,
    "ORBM_CULL_CODE_KEPT_FEW_KFS": CULL_CODE_KEPT_FEW_KFS, "ORBM_CULL_CODE_KEPT_RECENT": CULL_CODE_KEPT_RECENT,
    "ORBM_CULL_CODE_KEPT_NO_NEIGHBOUR": CULL_CODE_KEPT_NO_NEIGHBOUR, "ORBM_CULL_CODE_KEPT_INERTIAL": CULL_CODE_KEPT_INERTIAL,
    "ORBM_CULL_CODE_CULLED": CULL_CODE_CULLED, "ORBM_CULL_CODE_CULLED_IMU1": CULL_CODE_CULLED_IMU1,
    "ORBM_CULL_CODE_CULLED_IMU2": CULL_CODE_CULLED_IMU2, "ORBM_CULL_CODE_DEFERRED": CULL_CODE_DEFERRED,
    "ORBM_CULL_BAD_INDEX": CULL_BAD_INDEX, "ORBM_CULL_UNSUPPORTED": CULL_UNSUPPORTED, "ORBM_CULL_REC_LIVE": CULL_REC_LIVE,
    "ORBM_CULL_REC_ERASED_BY_KF": CULL_REC_ERASED_BY_KF, "ORBM_CULL_REC_ERASED_BY_POINT": CULL_REC_ERASED_BY_POINT,
    "ORBM_CULL_REC_ABSENT": CULL_REC_ABSENT,
    "ORBM_COVIS_KF_FIRST_CONNECTION": COVIS_KF_FIRST_CONNECTION, "ORBM_COVIS_BAD_INDEX": COVIS_BAD_INDEX, "ORBM_COVIS_OVERFLOW": COVIS_OVERFLOW,
    "ORBM_FUSENB_MONOCULAR": FUSENB_MONOCULAR, "ORBM_FUSENB_INERTIAL": FUSENB_INERTIAL, "ORBM_FUSENB_ABORT_BA": FUSENB_ABORT_BA,
    "ORBM_FUSENB_MAX_TARGETS": FUSENB_MAX_TARGETS, "ORBM_FUSENB_EV_ADD": FUSENB_EV_ADD, "ORBM_FUSENB_EV_LIST_POINT_REPLACED": FUSENB_EV_LIST_POINT_REPLACED,
    "ORBM_FUSENB_EV_KF_POINT_REPLACED": FUSENB_EV_KF_POINT_REPLACED, "ORBM_FUSENB_EV_NOOP_BAD": FUSENB_EV_NOOP_BAD,
    "ORBM_FUSENB_EV_NOOP_SAME": FUSENB_EV_NOOP_SAME, "ORBM_FUSENB_R_FLAGS": FUSENB_R_FLAGS, "ORBM_FUSENB_R_N_TARGETS": FUSENB_R_N_TARGETS,
    "ORBM_FUSENB_R_N_TARGETS_REQUIRED": FUSENB_R_N_TARGETS_REQUIRED, "ORBM_FUSENB_R_N_CANDIDATES": FUSENB_R_N_CANDIDATES,
    "ORBM_FUSENB_R_N_CANDIDATES_REQUIRED": FUSENB_R_N_CANDIDATES_REQUIRED, "ORBM_FUSENB_R_N_EVENTS": FUSENB_R_N_EVENTS,
    "ORBM_FUSENB_R_N_OBS": FUSENB_R_N_OBS, "ORBM_FUSENB_R_N_SEL": FUSENB_R_N_SEL, "ORBM_FUSENB_R_WORDS": FUSENB_R_WORDS,
    "ORBM_FUSENB_BAD_INDEX": FUSENB_BAD_INDEX, "ORBM_FUSENB_UNSUPPORTED": FUSENB_UNSUPPORTED,
    "ORBM_FUSENB_TARGET_OVERFLOW": FUSENB_TARGET_OVERFLOW, "ORBM_FUSENB_CANDIDATE_OVERFLOW": FUSENB_CANDIDATE_OVERFLOW,
    "ORBM_FUSENB_EVENT_OVERFLOW": FUSENB_EVENT_OVERFLOW, "ORBM_FUSENB_OBS_OVERFLOW": FUSENB_OBS_OVERFLOW,
    "ORBM_FUSENB_REFRESH_OVERFLOW": FUSENB_REFRESH_OVERFLOW, "ORBM_FUSENB_UNSORTED": FUSENB_UNSORTED,
    "ORBM_NEWKF_CODE_NOT_VISITED": NEWKF_CODE_NOT_VISITED, "ORBM_NEWKF_CODE_NONE": NEWKF_CODE_NONE,
    "ORBM_NEWKF_CODE_BAD_POINT": NEWKF_CODE_BAD_POINT, "ORBM_NEWKF_CODE_ADDED": NEWKF_CODE_ADDED, "ORBM_NEWKF_CODE_PUSHED": NEWKF_CODE_PUSHED,
    "ORBM_NEWKF_CODE_PUSHED_DUP": NEWKF_CODE_PUSHED_DUP, "ORBM_NEWKF_CODE_BAD_INDEX": NEWKF_CODE_BAD_INDEX,
    "ORBM_NEWKF_R_FLAGS": NEWKF_R_FLAGS, "ORBM_NEWKF_R_N_ADDED": NEWKF_R_N_ADDED, "ORBM_NEWKF_R_N_PUSHED": NEWKF_R_N_PUSHED,
    "ORBM_NEWKF_R_N_PUSH_REQUIRED": NEWKF_R_N_PUSH_REQUIRED, "ORBM_NEWKF_R_N_OBS": NEWKF_R_N_OBS, "ORBM_NEWKF_R_WORDS": NEWKF_R_WORDS,
    "ORBM_NEWKF_BAD_INDEX": NEWKF_BAD_INDEX, "ORBM_NEWKF_UNSUPPORTED": NEWKF_UNSUPPORTED, "ORBM_NEWKF_OBS_OVERFLOW": NEWKF_OBS_OVERFLOW,
    "ORBM_NEWKF_RECENT_OVERFLOW": NEWKF_RECENT_OVERFLOW, "ORBM_NEWKF_REFRESH_OVERFLOW": NEWKF_REFRESH_OVERFLOW,
    "ORBM_NEWKF_UNSORTED": NEWKF_UNSORTED, "ORBM_MPCULL_MONOCULAR": MPCULL_MONOCULAR,
    "ORBM_MPCULL_CODE_NOT_VISITED": MPCULL_CODE_NOT_VISITED, "ORBM_MPCULL_CODE_ERASED_BAD": MPCULL_CODE_ERASED_BAD,
    "ORBM_MPCULL_CODE_CULLED_RATIO": MPCULL_CODE_CULLED_RATIO, "ORBM_MPCULL_CODE_CULLED_OBS": MPCULL_CODE_CULLED_OBS,
    "ORBM_MPCULL_CODE_RETIRED": MPCULL_CODE_RETIRED, "ORBM_MPCULL_CODE_KEPT": MPCULL_CODE_KEPT,
    "ORBM_MPCULL_CODE_BAD_INDEX": MPCULL_CODE_BAD_INDEX,
    "ORBM_LBA_R_FLAGS": LBA_R_FLAGS, "ORBM_LBA_R_N_LOCAL": LBA_R_N_LOCAL, "ORBM_LBA_R_N_FIXED": LBA_R_N_FIXED,
    "ORBM_LBA_R_NUM_FIXED_KF": LBA_R_NUM_FIXED_KF, "ORBM_LBA_R_N_POINTS": LBA_R_N_POINTS, "ORBM_LBA_R_N_EDGES": LBA_R_N_EDGES,
    "ORBM_LBA_R_N_MONO": LBA_R_N_MONO, "ORBM_LBA_R_N_STEREO": LBA_R_N_STEREO, "ORBM_LBA_R_N_POSES_REQUIRED": LBA_R_N_POSES_REQUIRED,
    "ORBM_LBA_R_N_POINTS_REQUIRED": LBA_R_N_POINTS_REQUIRED, "ORBM_LBA_R_N_EDGES_REQUIRED": LBA_R_N_EDGES_REQUIRED,
    "ORBM_LBA_R_WORDS": LBA_R_WORDS, "ORBM_LBA_BAD_INDEX": LBA_BAD_INDEX, "ORBM_LBA_UNSUPPORTED": LBA_UNSUPPORTED,
    "ORBM_LBA_OVERFLOW": LBA_OVERFLOW, "ORBM_LBA_EARLY_RETURN": LBA_EARLY_RETURN, "ORBM_LBA_A_FLAGS": LBA_A_FLAGS,
    "ORBM_LBA_A_N_ERASED": LBA_A_N_ERASED, "ORBM_LBA_A_N_WENT_BAD": LBA_A_N_WENT_BAD, "ORBM_LBA_A_N_OBS": LBA_A_N_OBS,
    "ORBM_LBA_A_N_MONO": LBA_A_N_MONO, "ORBM_LBA_A_N_STEREO": LBA_A_N_STEREO, "ORBM_LBA_A_WORDS": LBA_A_WORDS,
    "BOWDB_KF_PRESENT": KF_PRESENT, "BOWDB_COVIS": COVIS, "BOWDB_MAX_CANDIDATES": MAX_CANDIDATES, "BOWDB_L1_NORM": BOWDB_L1_NORM,
    "LBA_EDGE_MONO": EDGE_MONO, "LBA_EDGE_STEREO": EDGE_STEREO, "LBA_EDGE_BODY": EDGE_BODY, "LBA_CAM_PINHOLE": CAM_PINHOLE, "LBA_CAM_KB8": CAM_KB8,
    "LBA_HINT_MONO_PINHOLE": HINT_MONO_PINHOLE, "LBA_HINT_PINHOLE": HINT_PINHOLE, "LIBA_MAX_FREE": LIBA_MAX_FREE, "LIBA_EDGE_CLOSE": EDGE_CLOSE,
}


def _prototypes():
    vp, i32, u32, sz, f32, f64, P = C.c_void_p, C.c_int, C.c_uint, C.c_size_t, C.c_float, C.c_double, C.POINTER
    lba, liba = P(LbaProblem), P(LibaProblem)
    return {
        "orbx_create": (i32, [P(OrbxConfig), i32, i32, i32, i32, P(vp)]),
        "orbx_destroy": (None, [vp]),
        "orbx_last_error": (C.c_char_p, [vp]),
        "orbx_get_tables": (i32, [vp, vp, vp, vp, vp, vp]),
        "orbx_max_keypoints": (i32, [vp]),
        "orbx_extract": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, P(i32), P(i32)]),
        "orbx_extract_view": (i32, [vp, vp, i32, i32, i32, i32, i32, P(vp), P(vp), P(i32), P(i32)]),
        "orbx_set_host_pyramid": (i32, [vp, i32]),
        "orbx_host_pyramid_level": (i32, [vp, i32, P(vp), P(i32), P(i32), P(i32)]),
        "orbx_extract_batch_dev": (i32, [vp, vp, i32, sz, i32, i32, i32, vp, vp, i32, vp, vp]),
        "orbx_pyramid_level": (i32, [vp, i32, i32, P(vp), P(i32), P(i32), P(i32)]),
        "orbx_copy_level": (i32, [vp, i32, i32, i32, vp]),
        "orbx_stereo_matches": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, vp]),
        "orbx_stereo_matches_last": (i32, [vp, vp, f32, f32, vp, vp, i32, P(i32)]),
        "orbx_debug_candidates": (i32, [vp, i32, i32, vp, i32, P(i32)]),
        "orbx_debug_selected": (i32, [vp, i32, i32, vp, i32, P(i32)]),
        "orbx_enable_timing": (i32, [vp, i32]),
        "orbx_last_timing": (i32, [vp, vp]),
        "orbx_last_fast_passes": (i32, [vp, vp, vp, vp]),
        "orbx_last_schedule": (i32, [vp, P(i32), P(i32)]),

        "orbm_hamming": (i32, [vp, i32, vp, i32, i32, vp, vp]),
        "orbm_knn2": (i32, [vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp]),
        "orbm_grid_build": (i32, [vp, vp, i32, i32, i32, P(GridParams), vp, vp, vp]),
        "orbm_search_workspace_bytes": (sz, [i32, i32]),
        "orbm_search_by_projection": (i32, [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, P(SearchParams), vp, vp, vp, vp, vp]),
        "orbm_search_by_bow": (i32, [P(BowSide), vp, P(BowSide), i32, f32, i32, vp, vp, vp]),
        "orbm_search_by_bow_kf": (i32, [P(BowSide), vp, P(BowSide), vp, i32, f32, i32, vp, vp, vp]),
        "orbm_enable_timing": (i32, [i32]),
        "orbm_last_timing": (i32, [vp]),
        "orbm_grid_build_rig": (i32, [vp, vp, vp, i32, i32, i32, P(GridParams), vp, vp, vp]),
        "orbm_search_by_projection_rig": (i32, [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, P(SearchParams), vp, vp, vp, vp, vp]),
        "orbm_fuse": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, P(FuseParams), vp, vp, vp, vp]),
        "orbm_search_for_triangulation": (i32, [P(TriSide), P(TriSide), vp, i32, i32, i32, i32, vp, vp, vp]),
        "orbm_search_for_triangulation_kb8": (i32, [P(TriSide), P(TriSide), vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "orbm_mutual_matches": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
        "orbm_predict_scale_thresholds": (i32, [f32, i32, vp]),
        "orbm_project_map_points": (i32, [vp, vp, i32, vp, vp, i32, P(ProjectParams), vp, vp, vp, vp, vp, vp, vp, i32, vp]),
        "orbm_refresh_map_points": (i32, [vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, i32, P(RefreshParams), vp, vp, vp]),
        "orbm_create_new_map_points": (i32, [P(NewPtSide), P(NewPtSide), vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        "orbm_append_new_map_points": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, vp, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp]),
        "orbm_local_map_workspace_bytes": (sz, [i32, i32, i32]),
        "orbm_update_local_map": (i32, [P(LocalMapView), vp, P(LocalMapLists), i32, P(LocalMapOut), vp, vp]),
        "orbm_store_local_tracks": (i32, [vp, vp, vp, i32, i32, vp, i32, i32, vp]),
        "orbm_cull_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "orbm_cull_workspace": (i32, [i32, i32, i32, P(CullWorkspaceLayout)]),
        "orbm_cull_keyframes": (i32, [P(LocalMapView), P(CullIn), i32, P(CullOut), vp, vp]),
        "orbm_apply_keyframe_culling": (i32, [P(LocalMapView), P(CullIn), i32, i32, P(CullApply), vp, vp]),
        "orbm_covis_workspace_bytes": (sz, [i32, i32]),
        "orbm_update_connections": (i32, [P(LocalMapView), P(CovisStore), vp, vp, vp, i32, u32, P(CovisOut), vp, vp]),
        "orbm_erase_connections": (i32, [P(LocalMapView), P(CovisStore), vp, vp, vp, vp, i32, P(CovisOut), vp, vp]),
        "orbm_fusenb_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32]),
        "orbm_search_in_neighbors": (i32, [P(LocalMapView), P(FuseNbIn), P(FuseNbParams), P(FuseNbOut), vp, vp]),
        "orbm_newkf_workspace_bytes": (sz, [i32, i32, i32]),
        "orbm_process_new_keyframe": (i32, [P(LocalMapView), P(NewKfIn), i32, P(RefreshParams), P(NewKfOut), vp, vp]),
        "orbm_recent_points_push": (i32, [vp, i32, vp, vp, i32, vp, vp]),
        "orbm_cull_map_points": (i32, [P(LocalMapView), P(NewKfIn), vp, i32, u32, vp, vp, P(MpCullOut), vp, vp]),
        "orbm_lba_workspace_bytes": (sz, [i32] * 8),
        "orbm_lba_window_build": (i32, [P(LocalMapView), P(LbaIn), i32, u32, P(LbaWindow), vp, vp]),
        "orbm_lba_window_apply": (i32, [P(LocalMapView), P(LbaIn), P(LbaWindow), vp, vp, P(LbaApply), vp, vp]),
        "orbm_sim3_ransac_iterations": (i32, [f64, i32, i32, i32]),
        "orbm_sim3_workspace_bytes": (sz, [i32, i32, i32]),
        "orbm_sim3_solve": (i32, [vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp]),
        "orbm_two_view_workspace_bytes": (sz, [i32, i32, i32]),
        "orbm_two_view_reconstruct": (i32, [vp, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),

        "orbf_undistort_keypoints": (i32, [vp, vp, i32, i32, i32, P(Camera), vp, vp]),
        "orbf_image_bounds": (i32, [P(Camera), i32, i32, P(f32 * 4), P(GridParams)]),
        "orbm_undistort_and_grid_build": (i32, [vp, vp, i32, i32, i32, P(Camera), P(GridParams), vp, vp, vp, vp]),
        "orbf_stereo_from_rgbd": (i32, [vp, vp, vp, i32, i32, i32, vp, sz, i32, i32, i32, f32, vp, vp, vp]),
        "orbf_stereo_fisheye_matches": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, P(FisheyeRig), vp, vp, vp, vp, vp, vp]),

        "bow_vocab_load_binary": (i32, [vp, sz, i32, P(vp)]),
        "bow_vocab_info": (i32, [vp, vp]),
        "bow_vocab_destroy": (None, [vp]),
        "bow_transform": (i32, [vp, vp, vp, i32, i32, i32, i32, P(BowResult), vp]),
        "bowdb_workspace_bytes": (sz, [i32, i32]),
        "bowdb_detect_relocalization_candidates": (i32, [P(View), vp, i32, P(QueryBows), vp, i32, vp, vp, vp, vp, vp]),
        "bowdb_detect_n_best_candidates": (i32, [P(View), vp, i32, P(QueryBows), vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]),

        "lba_build_system": (i32, [lba, i32, P(LbaSystem), vp]),
        "lba_build_system_hint": (i32, [lba, i32, P(LbaSystem), u32, vp]),
        "lba_compute_errors": (i32, [lba, i32, P(LbaSystem), vp]),
        "lba_lm_workspace_bytes": (sz, [lba, i32]),
        "lba_optimize": (i32, [lba, i32, i32, vp, vp, vp, vp]),
        "lba_optimize_stopflag": (i32, [lba, i32, i32, vp, vp, vp, vp]),
        "lba_optimize_sharded": (i32, [lba, i32, i32, vp, vp, i32, LBA_ALLREDUCE_FN, vp, vp]),
        "pose_optimize": (i32, [vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp]),
        "pose_optimize_hint": (i32, [vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, u32, vp]),

        "liba_workspace_bytes": (sz, [liba, i32]),
        "liba_optimize": (i32, [liba, i32, f64, i32, vp, vp, vp]),
        "liba_compute_errors": (i32, [liba, i32, vp, vp, vp, vp, vp]),
        "liba_pose_inertial_kf": (i32, [vp, vp, vp, i32, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp]),
        "liba_pose_inertial_lastframe": (i32, [vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp]),

        "orb_device_count": (i32, []),
        "orb_dev_alloc": (i32, [i32, sz, P(vp)]),
        "orb_dev_free": (i32, [vp]),
        "orb_host_alloc": (i32, [sz, P(vp)]),
        "orb_host_free": (i32, [vp]),
        "orb_memcpy_h2d": (i32, [vp, vp, sz, vp]),
        "orb_memcpy_d2h": (i32, [vp, vp, sz, vp]),
        "orb_memset": (i32, [vp, i32, sz, vp]),
        "orb_stream_sync": (i32, [vp]),
    }, {
        "orbd_allgather_frames": (i32, [vp, i32, i32, i32] + [vp] * 7),
        "orbd_allreduce_pose_system": (i32, [vp, vp, vp, i32, vp]),
        "orbd_allgather_pose_blocks": (i32, [vp, i32, vp, vp, i32, vp]),
        "orbd_ipc_export": (i32, [vp, vp]),
        "orbd_ipc_open": (i32, [vp, P(vp)]),
        "orbd_ipc_close": (i32, [vp]),
        "orbd_allgather_frames_peer": (i32, [i32, i32, i32, i32] + [vp] * 7),
        "orbd_peer_enable_access": (i32, [i32, P(i32)]),
        "orbd_peer_shutdown": (i32, []),
        "orbd_comm_init_all_local": (i32, [i32, P(i32), P(vp)]),
        "orbd_comm_destroy": (i32, [vp]),
    }


PROTOTYPES, ORBD_PROTOTYPES = _prototypes()   # name -> (restype, argtypes): every function of include/orbhip.h / include/orbd.h
