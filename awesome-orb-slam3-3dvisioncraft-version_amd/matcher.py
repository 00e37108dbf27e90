"""Host-side mirror of ORB_SLAM3::ORBmatcher (reference include/ORBmatcher.h:39-94) above the C ABI.

The reference methods take Frame&/KeyFrame*/MapPoint* pointer graphs; here they take the flattened records that the
C++ adapter gathers from those objects (include/orbhip.h "Stage 2"), batched over independent problems.  Arrays may be
torch CUDA tensors (product path) or numpy arrays (only meaningful with the emulated test build, whose "device" is
host memory).  Outputs are allocated like the inputs."""
import ctypes as C

import numpy as np

from . import _lib
from ._abi import (GRID_COLS, GRID_ROWS, HISTO_LENGTH, KEYFRAME_CENTER_DTYPE, MAP_POINT_DTYPE, MODE_BEST_ONLY, MODE_INIT, MODE_LOCAL_MAP,  # noqa: F401
                   MP_BAD, MP_HAS_OBS, MP_SEEN, MP_VALID, OBS_KF_BAD, OBS_RIGHT, OBSERVATION_DTYPE, PROJ_CAM_PINHOLE, PROJ_LAST_FRAME, PROJ_LOCAL_MAP,
                   PROJ_RELOC, PROJECT_FRAME_DTYPE, Q_HAS_OBS, Q_RIGHT, Q_STEREO, Q_TWIN, Q_VALID, QUERY_DTYPE, REFRESH_BAD_RECORD, REFRESH_DESCRIPTOR,
                   REFRESH_MAX_OBS, REFRESH_NORMAL_DEPTH, REFRESH_OVERFLOW, REFRESH_POINT_DTYPE, REFRESHED_DESCRIPTOR, REFRESHED_NORMAL_DEPTH,
                   TH_HIGH, TH_LOW, TRACK_DTYPE, TRI_KB8_PAIR_DTYPE, TRI_PAIR_DTYPE, BowSide, FuseParams, GridParams, ProjectParams, RefreshParams,
                   SearchParams, TriSide)
from ._abi import (NEW_POINT_DTYPE, NEWPT_BAD_INDEX, NEWPT_BEHIND_1, NEWPT_BEHIND_2, NEWPT_CAM_KB8, NEWPT_CAM_PINHOLE, NEWPT_CAMERA_DTYPE,  # noqa: F401
                   NEWPT_CREATED_STEREO1, NEWPT_CREATED_STEREO2, NEWPT_CREATED_TRIANGULATED, NEWPT_EMPTY_STEREO, NEWPT_FAR, NEWPT_LOW_PARALLAX,
                   NEWPT_NO_MATCH, NEWPT_PAIR_BAD_CAMERA, NEWPT_PAIR_BAD_INDEX, NEWPT_PAIR_DTYPE, NEWPT_PAIR_OVERFLOW, NEWPT_REPROJ_1,
                   NEWPT_REPROJ_2, NEWPT_SCALE, NEWPT_W_ZERO, NEWPT_ZERO_DIST, NewPtSide)
from ._abi import (LM_BAD_INDEX, LM_INERTIAL, LM_KF_BAD, LM_KF_OVERFLOW, LM_KF_PRESENT, LM_MP_OVERFLOW, LOCALMAP_FRAME_DTYPE,  # noqa: F401
                   LOCALMAP_KEYFRAME_DTYPE, LocalMapLists, LocalMapOut, LocalMapView)
from ._abi import (CULL_ABORT_BA, CULL_BAD_INDEX, CULL_CODE_CULLED, CULL_CODE_CULLED_IMU1, CULL_CODE_CULLED_IMU2, CULL_CODE_DEFERRED,  # noqa: F401
                   CULL_CODE_KEPT, CULL_CODE_KEPT_FEW_KFS, CULL_CODE_KEPT_INERTIAL, CULL_CODE_KEPT_NO_NEIGHBOUR, CULL_CODE_KEPT_RECENT,
                   CULL_CODE_NOT_VISITED, CULL_CODE_SKIPPED, CULL_EVENT_DTYPE, CULL_FEAT_CLOSE, CULL_FEAT_OCTAVE, CULL_FEAT_STEREO,
                   CULL_IMU_INITIALIZED, CULL_INERTIAL, CULL_INERTIAL_BA2, CULL_KEYFRAME_DTYPE, CULL_KF_NOT_ERASE, CULL_MONOCULAR,
                   CULL_PROBLEM_DTYPE, CULL_REC_ABSENT, CULL_REC_ERASED_BY_KF, CULL_REC_ERASED_BY_POINT, CULL_REC_LIVE, CULL_UNSUPPORTED,
                   CullApply, CullIn, CullOut, CullWorkspaceLayout)
from ._lib import OrbHipError, check, check_capacity, ptr, stream, to_host, zeros

_ptr = ptr   # the name earlier revisions of tests/test_map_refresh.py and tests/test_keyframe_database.py import from here


def flatten_observations(points):
    """points: per map point a list of (kf, desc_row, flags) in the order the reference visits them (mObservations' iteration order, left
    before right inside one entry).  -> (obs_start int32 [len + 1], obs OBSERVATION_DTYPE [total]) for RefreshMapPoints."""
    start = np.zeros(len(points) + 1, np.int32)
    start[1:] = np.cumsum([len(p) for p in points])
    obs = np.zeros(int(start[-1]), OBSERVATION_DTYPE)
    flat = [r for p in points for r in p]
    if flat:
        a = np.asarray(flat, np.int64).reshape(-1, 3)
        obs["kf"], obs["desc_row"], obs["flags"] = a[:, 0], a[:, 1], a[:, 2]
    return start, obs


def _addr(a):
    return None if a is None else ptr(a).value


def _nrec(a):
    """the number of records of a record array: numpy structured, or its uint8 [..., itemsize] view (torch has no structured dtypes)"""
    return int(a.size) if isinstance(a, np.ndarray) and a.dtype.names else int(np.prod(a.shape[:-1]))


def flatten_local_map_keyframes(keyframes):
    """keyframes: per key-frame slot None (an empty slot) or dict(bad, parent, prev, mp = GetMapPointMatches() as map-point indices (-1 = none),
    covis = GetBestCovisibilityKeyFrames(10), children = GetChilds() in the std::set's iteration order).
    -> (kf LOCALMAP_KEYFRAME_DTYPE [n], kf_mp int32 [rows], children int32 [total]) for UpdateLocalMap's view."""
    kf = np.zeros(len(keyframes), LOCALMAP_KEYFRAME_DTYPE)
    kf["parent"], kf["prev"], kf["covis"] = -1, -1, -1
    rows, children = [], []
    for i, k in enumerate(keyframes):
        if k is None:
            continue
        kf[i]["flags"] = LM_KF_PRESENT | (LM_KF_BAD if k.get("bad") else 0)
        kf[i]["parent"], kf[i]["prev"] = k.get("parent", -1), k.get("prev", -1)
        kf[i]["mp_row0"], kf[i]["n_feat"] = len(rows), len(k.get("mp", ()))
        rows.extend(k.get("mp", ()))
        cov = list(k.get("covis", ()))[:10]
        kf[i]["covis"][:len(cov)] = cov
        kf[i]["child_start"], kf[i]["n_child"] = len(children), len(k.get("children", ()))
        children.extend(k.get("children", ()))
    return kf, np.asarray(rows, np.int32).reshape(-1), np.asarray(children, np.int32).reshape(-1)


def flatten_cull_keyframes(keyframes):
    """keyframes: the list flatten_local_map_keyframes takes, every dict with the members the culling reads as well: id (mnId), prev / next
    (mPrevKF / mNextKF as indices, -1 = none), timestamp, imu_pos (GetImuPosition()), not_erase (mbNotErase), desc_row0 (default: the key
    frame's first row of kf_mp, i.e. one descriptor row per feature in key-frame order), octave (mvKeysUn[i].octave per feature), depth with
    th_depth (mvDepth, mThDepth) and u_right (mvuRight), all optional per feature list (default: octave 0, close, not stereo).  CLOSE is
    evaluated here with the reference's expression in float.  A rig (NLeft != -1 or camera2) is refused with ORB_E_INVALID.
    -> (ckf CULL_KEYFRAME_DTYPE [n], feat uint8 [rows]) parallel to the kf and kf_mp of flatten_local_map_keyframes."""
    ckf = np.zeros(len(keyframes), CULL_KEYFRAME_DTYPE)
    ckf["prev"], ckf["next"] = -1, -1
    feat = []
    for i, k in enumerate(keyframes):
        if k is None:
            continue
        if k.get("NLeft", -1) != -1 or k.get("camera2"):
            raise OrbHipError(_lib.ORB_E_INVALID, "key-frame culling: fisheye rigs (NLeft != -1, mpCamera2) are not supported")
        n = len(k.get("mp", ()))
        ckf[i]["timestamp"], ckf[i]["id"] = k.get("timestamp", 0.0), k.get("id", i)
        ckf[i]["prev"], ckf[i]["next"] = k.get("prev", -1), k.get("next", -1)
        ckf[i]["desc_row0"] = k.get("desc_row0", len(feat))
        ckf[i]["imu_pos"] = k.get("imu_pos", (0.0, 0.0, 0.0))
        ckf[i]["flags"] = CULL_KF_NOT_ERASE if k.get("not_erase") else 0
        octave = np.asarray(k.get("octave", [0] * n), np.int64).reshape(-1)
        if len(octave) != n or (n and (octave.min() < 0 or octave.max() > CULL_FEAT_OCTAVE)):
            raise OrbHipError(_lib.ORB_E_INVALID, "key-frame culling: one octave in [0, 64) per feature")
        b = octave.astype(np.uint8)
        if "depth" in k:
            d, th = np.asarray(k["depth"], np.float32), np.float32(k["th_depth"])
            b = b | np.where(~((d > th) | (d < 0)), CULL_FEAT_CLOSE, 0).astype(np.uint8)   # !(mvDepth[i] > mThDepth || mvDepth[i] < 0)
        else:
            b = b | np.uint8(CULL_FEAT_CLOSE)
        if "u_right" in k:
            b = b | np.where(np.asarray(k["u_right"], np.float32) >= 0, CULL_FEAT_STEREO, 0).astype(np.uint8)   # mvuRight[i] >= 0
        feat.extend(b.tolist())
    return ckf, np.asarray(feat, np.uint8).reshape(-1)


def _bow_side(d, n_left=False):
    """orbm_bow_side of dict(desc [B,cap,32], angle [B,cap], node_id [B,capn], node_start [B,capn+1], feat_idx [B,cap], n_nodes [B][, n_left [B]]);
    n_left is passed on only to the search that reads it."""
    return BowSide(_addr(d["desc"]), _addr(d["angle"]), _addr(d["node_id"]), _addr(d["node_start"]), _addr(d["feat_idx"]), _addr(d["n_nodes"]),
                   d["desc"].shape[1], d["node_id"].shape[1], _addr(d.get("n_left")) if n_left else None)


def _tri_side(d, u_right=False):
    """orbm_tri_side of dict(kps [B,cap,7], desc [B,cap,32], has_mp [B,cap] u8, node_id, node_start, feat_idx, n_nodes[, u_right [B,cap]])"""
    return TriSide(_addr(d["kps"]), _addr(d["desc"]), _addr(d.get("u_right")) if u_right else None, _addr(d["has_mp"]), _addr(d["node_id"]),
                   _addr(d["node_start"]), _addr(d["feat_idx"]), _addr(d["n_nodes"]), d["desc"].shape[1], d["node_id"].shape[1])


def _newpt_side(d):
    """orbm_newpt_side of dict(kps [B,cap,7], n [B][, kps_raw [B,cap,7], u_right [B,cap], depth [B,cap], has_mp [B,cap] u8])"""
    return NewPtSide(_addr(d["kps"]), _addr(d.get("kps_raw")), _addr(d.get("u_right")), _addr(d.get("depth")), _addr(d["n"]),
                     _addr(d.get("has_mp")), d["kps"].shape[1], 0)


def newpt_camera(Rcw, tcw, Ow, k, mb=0.0, mbf=0.0, level_sigma2=(), scale_factors=(), camera_type=NEWPT_CAM_PINHOLE, rig=False):
    """One orbm_newpt_camera (NEWPT_CAMERA_DTYPE scalar) from a key frame's pose and calibration: k = mvParameters (4 values for a pinhole, 8
    for KannalaBrandt8), invfx / invfy = 1.0f / fx, 1.0f / fy as the KeyFrame members are.  A fisheye rig (mpCamera2) or a camera type outside
    the two is refused with ORB_E_INVALID here, because the records are read on the device."""
    if rig or camera_type not in (NEWPT_CAM_PINHOLE, NEWPT_CAM_KB8) or len(level_sigma2) > 16 or len(scale_factors) > 16:
        raise OrbHipError(_lib.ORB_E_INVALID, "new map points: one pinhole or KannalaBrandt8 camera per key frame, at most 16 levels")
    c = np.zeros((), NEWPT_CAMERA_DTYPE)
    c["Rcw"], c["tcw"], c["Ow"] = np.asarray(Rcw, np.float32).reshape(9), np.asarray(tcw, np.float32), np.asarray(Ow, np.float32)
    c["camera_type"] = camera_type
    c["k"][:len(k)] = np.asarray(k, np.float32)
    c["invfx"], c["invfy"] = np.float32(1) / c["k"][0], np.float32(1) / c["k"][1]
    c["mb"], c["mbf"] = mb, mbf
    c["level_sigma2"][:len(level_sigma2)] = level_sigma2
    c["scale_factors"][:len(scale_factors)] = scale_factors
    return c


def newpt_pair(cam1, cam2, scale_factor, kf1=0, kf2=1, obs_kf2_first=False, desc_row0_1=0, desc_row0_2=0, bFarPoints=False, thFarPoints=0.0):
    """One orbm_newpt_pair: ratio_factor = 1.5f * mfScaleFactor of KF1 (LocalMapping.cc:562)."""
    p = np.zeros((), NEWPT_PAIR_DTYPE)
    p["cam1"], p["cam2"] = cam1, cam2
    p["ratio_factor"] = np.float32(1.5) * np.float32(scale_factor)
    p["far_points"], p["th_far_points"] = int(bool(bFarPoints)), thFarPoints
    p["kf1"], p["kf2"], p["obs_kf2_first"], p["desc_row0_1"], p["desc_row0_2"] = kf1, kf2, int(bool(obs_kf2_first)), desc_row0_1, desc_row0_2
    return p


class ORBmatcher:
    TH_HIGH, TH_LOW, HISTO_LENGTH = TH_HIGH, TH_LOW, HISTO_LENGTH

    def __init__(self, nnratio=0.6, checkOri=True, *, lib=None):   # ORBmatcher.h:39
        self.mfNNratio, self.mbCheckOrientation = float(nnratio), bool(checkOri)
        self._L = lib if lib is not None else _lib.load()

    def _check(self, rc):
        check(rc, "orbm call failed")

    # -- measurement facility: device time of the last grid build / projection search kernels (HIP events on the launch stream)
    def enable_timing(self, on=True):
        self._check(self._L.orbm_enable_timing(int(bool(on))))

    def last_timing(self):
        ms = np.zeros(3, np.float32)
        self._check(self._L.orbm_last_timing(ptr(ms)))
        return dict(grid_build=float(ms[0]), sbp_candidates=float(ms[1]), sbp_resolve=float(ms[2]))

    # -- ORBmatcher::DescriptorDistance for all pairs (ORBmatcher.cc:2700-2716): q [B,nq,32], t [B,nt,32] -> [B,nq,nt] uint16
    def DescriptorDistance(self, q, t):
        B, nq, _ = q.shape
        nt = t.shape[1]
        out = zeros(q, (B, nq, nt), np.uint16)
        self._check(self._L.orbm_hamming(ptr(q), nq, ptr(t), nt, B, ptr(out), stream(q)))
        return out

    # -- BFMatcher(NORM_HAMMING).knnMatch(k=2) (Frame.cc:1300): q [B,capq,32], nq [B] int32, t [B,capt,32], nt [B]
    def knnMatch2(self, q, nq, t, nt):
        B, capq, _ = q.shape
        idx = zeros(q, (B, capq, 2), np.int32)
        dist = zeros(q, (B, capq, 2), np.int32)
        self._check(self._L.orbm_knn2(ptr(q), ptr(nq), capq, ptr(t), ptr(nt), t.shape[1], 1, B, ptr(idx), ptr(dist), stream(q)))
        return idx, dist

    # -- Frame::AssignFeaturesToGrid (Frame.cc:444-478): kps [B,cap,7] f32 (orb_keypoint), counts int32 (stride in elements)
    def grid_build(self, kps, counts, grid, count_stride=1, out=None):
        B, cap = kps.shape[0], kps.shape[1]
        gs, gi = out if out is not None else (zeros(kps, (B, GRID_COLS * GRID_ROWS + 1), np.int32), zeros(kps, (B, cap), np.int32))
        gp = GridParams(*grid)
        self._check(self._L.orbm_grid_build(ptr(kps), ptr(counts), count_stride, cap, B, C.byref(gp), ptr(gs), ptr(gi), stream(kps)))
        return gs, gi

    # -- SearchByProjection (ORBmatcher.cc:59-255 mode LOCAL_MAP / :2244-2509 mode BEST_ONLY) on flattened records
    def SearchByProjection(self, kps, desc, counts, grid_start, grid_idx, queries, qdesc, nq, grid, mode, th_dist=TH_HIGH,
                           u_right=None, occupied0=None, count_stride=1, work=None, out=None):
        """out = (q_match [B,cap_q], kp_match [B,cap_k], nmatches [B]) int32 buffers of an earlier call may be passed back in (every entry is rewritten)."""
        B, cap_k = kps.shape[0], kps.shape[1]
        cap_q = qdesc.shape[1]
        q_match, kp_match, nmatches = out if out is not None else (zeros(kps, (B, cap_q), np.int32), zeros(kps, (B, cap_k), np.int32), zeros(kps, (B,), np.int32))
        if work is None:
            work = zeros(kps, (self._L.orbm_search_workspace_bytes(B, cap_q),), np.uint8)
        prm = SearchParams(mode, th_dist, self.mfNNratio, int(self.mbCheckOrientation), GridParams(*grid))
        self._check(self._L.orbm_search_by_projection(ptr(kps), ptr(desc), ptr(u_right), ptr(occupied0), ptr(counts), count_stride,
                                                      cap_k, ptr(grid_start), ptr(grid_idx), ptr(queries), ptr(qdesc), ptr(nq),
                                                      cap_q, B, C.byref(prm), ptr(q_match), ptr(kp_match), ptr(nmatches),
                                                      ptr(work), stream(kps)))
        return q_match, kp_match, nmatches

    # -- fisheye rig (Nleft != -1): kps/desc = [left | right] concatenated, n_left [B]; grid with 2*64*48 cells
    def grid_build_rig(self, kps, counts, n_left, grid, count_stride=1):
        B, cap = kps.shape[0], kps.shape[1]
        gs = zeros(kps, (B, 2 * GRID_COLS * GRID_ROWS + 1), np.int32)
        gi = zeros(kps, (B, cap), np.int32)
        gp = GridParams(*grid)
        self._check(self._L.orbm_grid_build_rig(ptr(kps), ptr(counts), ptr(n_left), count_stride, cap, B, C.byref(gp), ptr(gs), ptr(gi),
                                                stream(kps)))
        return gs, gi

    def SearchByProjectionRig(self, kps, desc, counts, grid_start, grid_idx, queries, qdesc, nq, grid, mode, th_dist=TH_HIGH, kp_link=None,
                              occupied0=None, count_stride=1):
        """Rig twins of SearchByProjection (ORBmatcher.cc:184-251 / :2403-2460): queries in map-point order, a right-camera query flagged
        Q_RIGHT | Q_TWIN directly after its left one."""
        B, cap_k = kps.shape[0], kps.shape[1]
        cap_q = qdesc.shape[1]
        q_match = zeros(kps, (B, cap_q), np.int32)
        kp_match = zeros(kps, (B, cap_k), np.int32)
        nmatches = zeros(kps, (B,), np.int32)
        work = zeros(kps, (self._L.orbm_search_workspace_bytes(B, cap_q),), np.uint8)
        prm = SearchParams(mode, th_dist, self.mfNNratio, int(self.mbCheckOrientation), GridParams(*grid))
        self._check(self._L.orbm_search_by_projection_rig(ptr(kps), ptr(desc), ptr(occupied0), ptr(kp_link), ptr(counts), count_stride, cap_k,
                                                          ptr(grid_start), ptr(grid_idx), ptr(queries), ptr(qdesc), ptr(nq), cap_q, B,
                                                          C.byref(prm), ptr(q_match), ptr(kp_match), ptr(nmatches), ptr(work), stream(kps)))
        return q_match, kp_match, nmatches

    # -- SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORBmatcher.cc:323-587) on FeatureVector CSRs
    def SearchByBoW(self, kf, kf_valid, f):
        """kf / f: dict(desc [B,cap,32], angle [B,cap], node_id [B,capn], node_start [B,capn+1], feat_idx [B,cap], n_nodes [B])"""
        B = kf["desc"].shape[0]
        f_match = zeros(f["desc"], (B, f["desc"].shape[1]), np.int32)
        nmatches = zeros(f["desc"], (B,), np.int32)
        a, b = _bow_side(kf, n_left=True), _bow_side(f, n_left=True)
        self._check(self._L.orbm_search_by_bow(C.byref(a), ptr(kf_valid), C.byref(b), B, self.mfNNratio, int(self.mbCheckOrientation),
                                               ptr(f_match), ptr(nmatches), stream(f["desc"])))
        return f_match, nmatches

    # -- SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (ORBmatcher.cc:984-1124; LoopClosing.cc:697) on FeatureVector CSRs
    def SearchByBoWKF(self, kf1, valid1, kf2, valid2):
        """kf1 / kf2 as in SearchByBoW; valid1 / valid2 [B,cap] u8 = feature holds a good map point (and is a left-camera feature on a rig).
        -> (vpMatches12 as indices into key frame 2 or -1 [B,cap1] int32, nmatches [B])"""
        B = kf1["desc"].shape[0]
        m12 = zeros(kf1["desc"], (B, kf1["desc"].shape[1]), np.int32)
        nmatches = zeros(kf1["desc"], (B,), np.int32)
        a, b = _bow_side(kf1), _bow_side(kf2)
        self._check(self._L.orbm_search_by_bow_kf(C.byref(a), ptr(valid1), C.byref(b), ptr(valid2), B, self.mfNNratio,
                                                  int(self.mbCheckOrientation), ptr(m12), ptr(nmatches), stream(kf1["desc"])))
        return m12, nmatches

    # -- SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORBmatcher.cc:838-979)
    def SearchForInitialization(self, kps1, desc1, n1, kps2, desc2, n2, grid_start2, grid_idx2, prev_matched, grid, windowSize=10):
        """kps1/kps2 [B,cap,7] f32 (mvKeysUn), prev_matched [B,cap1,2] f32 (vbPrevMatched, updated in place like the reference).
        -> (vnMatches12 [B,cap1] int32, nmatches [B])"""
        B, cap1 = kps1.shape[0], kps1.shape[1]
        if isinstance(kps1, np.ndarray):
            q = np.zeros((B, cap1), QUERY_DTYPE)
            q["u"], q["v"], q["radius"], q["angle"] = prev_matched[..., 0], prev_matched[..., 1], float(windowSize), kps1[..., 3]
            q["flags"] = np.where(kps1.view(np.int32)[..., 5] == 0, Q_VALID, 0)
            queries = q.view(np.uint8).reshape(B, -1)
        else:
            import torch
            q = torch.zeros((B, cap1, 7), dtype=torch.float32, device=kps1.device)
            q[..., 0], q[..., 1], q[..., 2], q[..., 4] = prev_matched[..., 0], prev_matched[..., 1], float(windowSize), kps1[..., 3]
            q.view(torch.int32)[..., 6] = (kps1.view(torch.int32)[..., 5] == 0).to(torch.int32) * Q_VALID
            queries = q
        q_match, _, nm = self.SearchByProjection(kps2, desc2, n2, grid_start2, grid_idx2, queries, desc1, n1, grid, MODE_INIT, TH_LOW)
        # :972-975  vbPrevMatched[i1] = F2.mvKeysUn[vnMatches12[i1]].pt for the matched ones
        if isinstance(kps1, np.ndarray):
            bi, qi = np.nonzero(q_match >= 0)
            prev_matched[bi, qi] = kps2[bi, q_match[bi, qi], :2]
        else:
            import torch
            bi, qi = torch.nonzero(q_match >= 0, as_tuple=True)
            prev_matched[bi, qi] = kps2[bi, q_match[bi, qi].long(), :2]
        return q_match, nm

    # -- Fuse (search half; ORBmatcher.cc:1630-1882 with chi2_gate, :1884-2006 without)
    def Fuse(self, kps, desc, counts, grid_start, grid_idx, queries, qdesc, nq, grid, inv_level_sigma2=None, u_right=None, th_dist=TH_LOW,
             count_stride=1):
        B, cap_k = kps.shape[0], kps.shape[1]
        cap_q = qdesc.shape[1]
        q_match = zeros(kps, (B, cap_q), np.int32)
        q_dist = zeros(kps, (B, cap_q), np.int32)
        nfused = zeros(kps, (B,), np.int32)
        prm = FuseParams(th_dist, 0 if inv_level_sigma2 is None else 1, GridParams(*grid),
                         (C.c_float * 16)(*([float(v) for v in inv_level_sigma2] + [0.0] * 16)[:16] if inv_level_sigma2 is not None else [0.0] * 16))
        self._check(self._L.orbm_fuse(ptr(kps), ptr(desc), ptr(u_right), ptr(counts), count_stride, cap_k, ptr(grid_start), ptr(grid_idx),
                                      ptr(queries), ptr(qdesc), ptr(nq), cap_q, B, C.byref(prm), ptr(q_match), ptr(q_dist), ptr(nfused),
                                      stream(kps)))
        return q_match, q_dist, nfused

    # -- SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (ORBmatcher.cc:2008-2220)
    def SearchBySim3(self, kf1, kf2, q12, q12desc, q21, q21desc):
        """kf1 / kf2: dict(kps [B,cap,7], desc, counts [B], grid_start, grid_idx, grid).  q12[b][i1] = map point of key frame 1's keypoint i1
        projected into key frame 2 (VALID iff it exists, is not already matched and passed the gates of :2044-2080); q21 likewise the other
        way.  One query slot per keypoint (cap_q = cap_k).  -> (vpMatches12 as indices into key frame 2 or -1 [B,cap1], nFound [B])"""
        n1, n2 = kf1["counts"], kf2["counts"]
        m12, _, _ = self.Fuse(kf2["kps"], kf2["desc"], n2, kf2["grid_start"], kf2["grid_idx"], q12, q12desc, n1, kf2["grid"], th_dist=TH_HIGH)
        m21, _, _ = self.Fuse(kf1["kps"], kf1["desc"], n1, kf1["grid_start"], kf1["grid_idx"], q21, q21desc, n2, kf1["grid"], th_dist=TH_HIGH)
        B, cap1, cap2 = m12.shape[0], m12.shape[1], m21.shape[1]
        out = zeros(m12, (B, cap1), np.int32)
        nfound = zeros(m12, (B,), np.int32)
        self._check(self._L.orbm_mutual_matches(ptr(m12), ptr(m21), ptr(n1), ptr(n2), cap1, cap2, B, ptr(out), ptr(nfound), stream(m12)))
        return out, nfound

    # -- SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) (ORBmatcher.cc:1138-1428), pinhole / one camera
    def SearchForTriangulation(self, kf1, kf2, pairs, bOnlyStereo=False, bCoarse=False):
        """kf1 / kf2: dict(kps [B,cap,7], desc [B,cap,32], u_right [B,cap] or None, has_mp [B,cap] u8, node_id, node_start, feat_idx, n_nodes);
        pairs: u8 view of TRI_PAIR_DTYPE[B].  -> (vMatches12 [B,cap1] int32, nmatches [B])"""
        B = kf1["desc"].shape[0]
        m12 = zeros(kf1["desc"], (B, kf1["desc"].shape[1]), np.int32)
        nm = zeros(kf1["desc"], (B,), np.int32)
        a, b = _tri_side(kf1, u_right=True), _tri_side(kf2, u_right=True)
        self._check(self._L.orbm_search_for_triangulation(C.byref(a), C.byref(b), ptr(pairs), B, int(bOnlyStereo), int(bCoarse),
                                                          int(self.mbCheckOrientation), ptr(m12), ptr(nm), stream(kf1["desc"])))
        return m12, nm

    # -- SearchForTriangulation on KannalaBrandt8 key frames (monocular fisheye or rig with mpCamera2): ORBmatcher.cc:1138-1428 rig branches
    def SearchForTriangulationKB8(self, kf1, kf2, n_left1, n_left2, pairs, bOnlyStereo=False, bCoarse=False):
        """kf1 / kf2 as in SearchForTriangulation with kps = [mvKeys | mvKeysRight] (u_right ignored); n_left* [B] int32 (NLeft; unused when
        n_cams = 1); pairs: u8 view of TRI_KB8_PAIR_DTYPE[B].  -> (vMatches12 [B,cap1] int32, nmatches [B])"""
        B = kf1["desc"].shape[0]
        m12 = zeros(kf1["desc"], (B, kf1["desc"].shape[1]), np.int32)
        nm = zeros(kf1["desc"], (B,), np.int32)
        a, b = _tri_side(kf1), _tri_side(kf2)
        self._check(self._L.orbm_search_for_triangulation_kb8(C.byref(a), C.byref(b), ptr(n_left1), ptr(n_left2), ptr(pairs), B, int(bOnlyStereo),
                                                              int(bCoarse), int(self.mbCheckOrientation), ptr(m12), ptr(nm), stream(kf1["desc"])))
        return m12, nm

    # -- map-point projection (include/orbhip.h "Map-point projection"): isInFrustum / PredictScale / the query loops of SearchByProjection
    def PredictScaleThresholds(self, log_scale_factor, nlevels):
        """MapPoint::PredictScale's level steps for mfLogScaleFactor: float32 [nlevels - 1], made with the host's logf."""
        t = np.zeros(16, np.float32)
        self._check(self._L.orbm_predict_scale_thresholds(float(log_scale_factor), int(nlevels), ptr(t)))
        return t[:max(int(nlevels) - 1, 0)]

    def ProjectParams(self, mode, camera, scale_factors, log_scale_factor, th, mbf=0.0, mb=0.0, bMono=True, viewingCosLimit=0.5,
                      bFarPoints=False, thFarPoints=0.0, n_desc_rows=0):
        """The orbm_project_params of one call: camera = (fx, fy, cx, cy) of a pinhole camera, scale_factors = mvScaleFactors."""
        sf = [float(v) for v in scale_factors]
        p = ProjectParams()
        p.mode, p.camera_type, p.nleft = int(mode), PROJ_CAM_PINHOLE, -1
        p.fx, p.fy, p.cx, p.cy = [float(v) for v in camera]
        p.mbf, p.mb, p.mono, p.th, p.view_cos_limit = float(mbf), float(mb), int(bool(bMono)), float(th), float(viewingCosLimit)
        p.far_points, p.th_far_points, p.nlevels, p.n_desc_rows = int(bool(bFarPoints)), float(thFarPoints), len(sf), int(n_desc_rows)
        for i, v in enumerate(sf[:16]):
            p.scale_factors[i] = v
        for i, v in enumerate(self.PredictScaleThresholds(log_scale_factor, len(sf))):
            p.level_thresholds[i] = float(v)
        return p

    def ProjectMapPoints(self, mp, nmp, mp_desc, frames, params, cap_q, track=None, out=None):
        """Projects the map-point lists of B frames into query records (orbm_project_map_points), asynchronously on the inputs' stream.
        mp: MAP_POINT_DTYPE records [B, cap_mp] (torch: uint8 [B, cap_mp, 48]); nmp [B] int32; mp_desc [rows, 32] uint8 (desc_row indexes it);
        frames: PROJECT_FRAME_DTYPE [B] (torch: uint8 [B, 124]); params: ProjectParams (n_desc_rows is taken from mp_desc);
        track: TRACK_DTYPE [B, cap_mp] (torch: uint8 [B, cap_mp, 32]), in/out, LOCAL_MAP only.
        out: a dict of an earlier call to write into (same shapes).  -> dict(queries [B, cap_q, 28] u8 view of QUERY_DTYPE, qdesc [B, cap_q, 32],
        nq [B], q_src [B, cap_q], n_required [B], n_in_view [B], track, cap_q).  nq is capped at cap_q: check_overflow() reports a shortfall."""
        B, cap_mp = mp.shape[0], mp.shape[1]
        prm = ProjectParams.from_buffer_copy(params)
        prm.n_desc_rows = int(mp_desc.shape[0])
        if out is None:
            out = dict(queries=zeros(mp, (B, cap_q, QUERY_DTYPE.itemsize), np.uint8), qdesc=zeros(mp, (B, cap_q, 32), np.uint8),
                       nq=zeros(mp, (B,), np.int32), q_src=zeros(mp, (B, cap_q), np.int32), n_required=zeros(mp, (B,), np.int32),
                       n_in_view=zeros(mp, (B,), np.int32))
        out["track"], out["cap_q"] = track, int(cap_q)
        self._check(self._L.orbm_project_map_points(ptr(mp), ptr(nmp), cap_mp, ptr(mp_desc), ptr(frames), B, C.byref(prm), ptr(track),
                                                    ptr(out["queries"]), ptr(out["qdesc"]), ptr(out["nq"]), ptr(out["q_src"]),
                                                    ptr(out["n_required"]), ptr(out["n_in_view"]), int(cap_q), stream(mp)))
        return out

    def check_overflow(self, proj):
        """Host check (reads n_required back): raises OrbHipError(ORB_E_CAPACITY) if any frame produced more queries than cap_q."""
        req = to_host(proj["n_required"])
        bad = np.nonzero(req > proj["cap_q"])[0]
        check_capacity(bad, lambda b: "projection: %d frame(s) need more than cap_q = %d queries (frame %d: %d)"
                       % (len(bad), proj["cap_q"], b, int(req[b])))

    def SearchByProjectionFromMap(self, kps, desc, counts, grid_start, grid_idx, grid, mp, nmp, mp_desc, frames, params, cap_q, track=None,
                                  th_dist=TH_HIGH, u_right=None, occupied0=None, count_stride=1, work=None, out=None):
        """ProjectMapPoints followed by SearchByProjection on one stream, no host reads (a single-stream graph capture records both launches).
        The search mode follows the projection: LOCAL_MAP -> MODE_LOCAL_MAP, LAST_FRAME / RELOC -> MODE_BEST_ONLY (th_dist = ORBdist for RELOC).
        out / work: the buffers of an earlier call (every entry is rewritten).  -> dict of ProjectMapPoints plus q_match, kp_match (query indices),
        kp_match_mp (map-point indices: q_src[kp_match] where kp_match >= 0, else kp_match) and nmatches."""
        B, cap_k = kps.shape[0], kps.shape[1]
        proj = self.ProjectMapPoints(mp, nmp, mp_desc, frames, params, cap_q, track=track, out=out)
        if "q_match" not in proj:
            proj.update(q_match=zeros(kps, (B, cap_q), np.int32), kp_match=zeros(kps, (B, cap_k), np.int32), nmatches=zeros(kps, (B,), np.int32),
                        kp_match_mp=zeros(kps, (B, cap_k), np.int32))
        mode = MODE_LOCAL_MAP if params.mode == PROJ_LOCAL_MAP else MODE_BEST_ONLY
        self.SearchByProjection(kps, desc, counts, grid_start, grid_idx, proj["queries"], proj["qdesc"], proj["nq"], grid, mode, th_dist,
                                u_right=u_right, occupied0=occupied0, count_stride=count_stride, work=work,
                                out=(proj["q_match"], proj["kp_match"], proj["nmatches"]))
        km, src, dst = proj["kp_match"], proj["q_src"], proj["kp_match_mp"]
        if isinstance(km, np.ndarray):
            dst[...] = np.where(km >= 0, np.take_along_axis(src, np.maximum(km, 0), 1), km)
        else:
            import torch
            torch.where(km >= 0, torch.gather(src, 1, km.clamp(min=0).long()), km, out=dst)
        return proj

    # -- map-point refresh (include/orbhip.h "Map-point refresh"): ComputeDistinctiveDescriptors / UpdateNormalAndDepth on device records
    def RefreshParams(self, scale_factors, what=REFRESH_DESCRIPTOR | REFRESH_NORMAL_DEPTH):
        """The orbm_refresh_params of one call: scale_factors = mvScaleFactors of the reference key frames (nlevels = its length)."""
        sf = [float(v) for v in scale_factors]
        p = RefreshParams()
        p.what, p.nlevels = int(what), len(sf)
        for i, v in enumerate(sf[:16]):
            p.scale_factors[i] = v
        return p

    def RefreshMapPoints(self, mp, mp_desc, obs_start, obs, ref, kf, kf_desc, params, sel=None, out=None):
        """Recomputes the representative descriptor and / or normal, min_distance, max_distance of the selected map points
        (orbm_refresh_map_points), asynchronously on the inputs' stream; mp and mp_desc are updated in place.
        mp: MAP_POINT_DTYPE records (torch: uint8 [..., 48]); mp_desc [rows, 32] uint8; obs_start int32 [n_mp + 1] and obs OBSERVATION_DTYPE
        (torch: uint8 [total, 12]): see flatten_observations; ref: REFRESH_POINT_DTYPE [n_mp] (torch: uint8 [n_mp, 8]); kf:
        KEYFRAME_CENTER_DTYPE [n_kf] (torch: uint8 [n_kf, 24]); kf_desc [rows, 32] uint8; params: RefreshParams; sel: int32 indices of the
        points to refresh (None: all).  out: the dict of an earlier call to write into.
        -> dict(best_obs int32 [n_mp], status int32 [n_mp] of REFRESH* bits); only the entries of selected points are written.
        A point with more than REFRESH_MAX_OBS usable records is left untouched and flagged: check_refresh_overflow() reports it."""
        n_mp = mp.size if isinstance(mp, np.ndarray) and mp.dtype.names else int(np.prod(mp.shape[:-1]))
        n_kf = kf.size if isinstance(kf, np.ndarray) and kf.dtype.names else int(np.prod(kf.shape[:-1]))
        if obs_start.shape[0] != n_mp + 1 or ref.shape[0] != n_mp:
            raise OrbHipError(_lib.ORB_E_INVALID, "RefreshMapPoints: obs_start needs n_mp + 1 entries and ref n_mp")
        if out is None:
            out = dict(best_obs=zeros(mp_desc, (n_mp,), np.int32), status=zeros(mp_desc, (n_mp,), np.int32))
        prm = RefreshParams.from_buffer_copy(params)
        self._check(self._L.orbm_refresh_map_points(ptr(mp), n_mp, ptr(mp_desc), int(mp_desc.shape[0]), ptr(sel),
                                                    0 if sel is None else int(sel.shape[0]), ptr(obs_start), ptr(obs), ptr(ref), ptr(kf), n_kf,
                                                    ptr(kf_desc), int(kf_desc.shape[0]), C.byref(prm), ptr(out["best_obs"]), ptr(out["status"]),
                                                    stream(mp_desc)))
        return out

    def check_refresh_overflow(self, refreshed, sel=None):
        """Host check (reads status back): raises OrbHipError(ORB_E_CAPACITY) if a refreshed point (those of sel; None: all) had more than
        REFRESH_MAX_OBS usable observation records and was therefore left untouched."""
        st = to_host(refreshed["status"])
        if sel is not None:
            sel = to_host(sel)
        idx = np.arange(len(st)) if sel is None else sel[(sel >= 0) & (sel < len(st))]
        bad = idx[(st[idx] & REFRESH_OVERFLOW) != 0]
        check_capacity(bad, lambda b: "refresh: %d map point(s) have more than %d usable observations (first: point %d)"
                       % (len(bad), REFRESH_MAX_OBS, b))

    # -- new map points (include/orbhip.h "New map points"): the loop of LocalMapping::CreateNewMapPoints behind SearchForTriangulation
    def CreateNewMapPoints(self, kf1, kf2, pairs, match12, cap_new, out=None):
        """LocalMapping.cc:651-904 for B (KF1, KF2) pairs in one launch (orbm_create_new_map_points), asynchronously on the inputs' stream.
        kf1 / kf2: dict(kps [B,cap,7] mvKeysUn, n [B] int32, optional kps_raw [B,cap,7] mvKeys, u_right + depth [B,cap] (absent / None =
        monocular), has_mp [B,cap] u8 (in/out; absent / None = not updated)): the dicts SearchForTriangulation takes fit once `n` is added.
        pairs: u8 view of NEWPT_PAIR_DTYPE[B] (newpt_camera / newpt_pair build them and refuse what the kernel does not cover);
        match12 [B,cap1] int32 as SearchForTriangulation returns it.  out: the dict of an earlier call to write into.
        -> dict(status [B,cap1] u8 of NEWPT_* codes, new [B,cap_new,24] u8 view of NEW_POINT_DTYPE, nnew [B], nrequired [B],
        point_of_1 [B,cap1], point_of_2 [B,cap2], pair_flags [B] int32 of NEWPT_PAIR_* bits, cap_new).  nnew is capped at cap_new:
        check_new_points() reports a shortfall."""
        B, cap1, cap2 = kf1["kps"].shape[0], kf1["kps"].shape[1], kf2["kps"].shape[1]
        like = kf1["kps"]
        if out is None:
            out = dict(status=zeros(like, (B, cap1), np.uint8), new=zeros(like, (B, cap_new, NEW_POINT_DTYPE.itemsize), np.uint8),
                       nnew=zeros(like, (B,), np.int32), nrequired=zeros(like, (B,), np.int32), point_of_1=zeros(like, (B, cap1), np.int32),
                       point_of_2=zeros(like, (B, cap2), np.int32), pair_flags=zeros(like, (B,), np.int32))
        out["cap_new"] = int(cap_new)
        a, b = _newpt_side(kf1), _newpt_side(kf2)
        self._check(self._L.orbm_create_new_map_points(C.byref(a), C.byref(b), ptr(pairs), ptr(match12), B, ptr(out["status"]), ptr(out["new"]),
                                                       int(cap_new), ptr(out["nnew"]), ptr(out["nrequired"]), ptr(out["point_of_1"]),
                                                       ptr(out["point_of_2"]), ptr(out["pair_flags"]), stream(like)))
        return out

    def check_new_points(self, created):
        """Host check (reads nrequired / pair_flags back): raises OrbHipError(ORB_E_CAPACITY) if a pair created more points than cap_new,
        OrbHipError(ORB_E_INVALID) if a pair was flagged for an index out of range or a camera type the kernel does not cover."""
        req, fl = to_host(created["nrequired"]), to_host(created["pair_flags"])
        bad = np.nonzero(fl & (NEWPT_PAIR_BAD_INDEX | NEWPT_PAIR_BAD_CAMERA))[0]
        if len(bad):
            raise OrbHipError(_lib.ORB_E_INVALID, "new map points: %d pair(s) flagged (pair %d: flags %d)" % (len(bad), bad[0], int(fl[bad[0]])))
        over = np.nonzero(req > created["cap_new"])[0]
        check_capacity(over, lambda b: "new map points: %d pair(s) need more than cap_new = %d points (pair %d: %d)"
                       % (len(over), created["cap_new"], b, int(req[b])))

    def AppendNewMapPoints(self, created, pairs, kps1, n_mp, mp, mp_desc_rows, obs_start, obs, ref, cap_sel, out=None):
        """Appends the points of CreateNewMapPoints to the device map behind the cursor n_mp (orbm_append_new_map_points), in order, on the
        inputs' stream.  created: the dict CreateNewMapPoints returned; pairs / kps1: as given to it; n_mp: int32 [1], in/out; mp:
        MAP_POINT_DTYPE records [cap_mp] (torch: uint8 [cap_mp, 48]); mp_desc_rows: the rows of the map-point descriptor slab; obs_start int32
        [cap_mp + 1]; obs: OBSERVATION_DTYPE [cap_obs] (torch: uint8 [cap_obs, 12]); ref: REFRESH_POINT_DTYPE [cap_mp].
        -> dict(sel int32 [cap_sel]: the new indices then -1, appended int32 [2]: written, shortfall).  RefreshMapPoints(..., sel=sel) may follow."""
        cap_mp = mp.size if isinstance(mp, np.ndarray) and mp.dtype.names else int(np.prod(mp.shape[:-1]))
        cap_obs = obs.size if isinstance(obs, np.ndarray) and obs.dtype.names else int(np.prod(obs.shape[:-1]))
        if obs_start.shape[0] != cap_mp + 1 or ref.shape[0] != cap_mp:
            raise OrbHipError(_lib.ORB_E_INVALID, "AppendNewMapPoints: obs_start needs cap_mp + 1 entries and ref cap_mp")
        if out is None:
            out = dict(sel=zeros(kps1, (cap_sel,), np.int32), appended=zeros(kps1, (2,), np.int32))
        B, cap_new = created["new"].shape[0], created["new"].shape[1]
        self._check(self._L.orbm_append_new_map_points(ptr(created["new"]), ptr(created["nnew"]), cap_new, ptr(pairs), B, ptr(kps1),
                                                       kps1.shape[1], ptr(n_mp), ptr(mp), cap_mp, int(mp_desc_rows), ptr(obs_start), ptr(obs),
                                                       cap_obs, ptr(ref), ptr(out["sel"]), int(out["sel"].shape[0]), ptr(out["appended"]),
                                                       stream(kps1)))
        return out

    def check_appended(self, appended):
        """Host check: raises OrbHipError(ORB_E_CAPACITY) if AppendNewMapPoints could not write every point."""
        a = to_host(appended["appended"])
        check_capacity([0] if a[1] else [], lambda _: "append: %d new map point(s) did not fit (%d written)" % (int(a[1]), int(a[0])))

    # -- local map (include/orbhip.h "Local map"): Tracking::UpdateLocalMap on the device map
    def LocalMapWorkspace(self, view, batch):
        """int32 workspace of UpdateLocalMap for the view's sizes, allocated like the view's arrays"""
        n = self._L.orbm_local_map_workspace_bytes(_nrec(view["kf"]), _nrec(view["mp"]), int(batch))
        return zeros(view["kf_by_order"], (max(n // 4, 1),), np.int32)

    @staticmethod
    def _local_map_view(view):
        """orbm_localmap_view of dict(mp MAP_POINT_DTYPE [n_mp], obs_start int32 [n_mp + 1], obs OBSERVATION_DTYPE, kf LOCALMAP_KEYFRAME_DTYPE
        [n_kf], kf_mp int32, children int32, kf_by_order int32 [n_kf], mp_track TRACK_DTYPE [n_mp] (one frame) or [B, n_mp]); record arrays
        are uint8 [..., itemsize] views under torch."""
        mp, trk = view["mp"], view["mp_track"]
        n_mp, n_kf = _nrec(mp), _nrec(view["kf"])
        batched = trk.ndim == (2 if isinstance(trk, np.ndarray) and trk.dtype.names else 3)
        if view["obs_start"].shape[0] != n_mp + 1 or view["kf_by_order"].shape[0] != n_kf or _nrec(trk) != n_mp * (trk.shape[0] if batched else 1):
            raise OrbHipError(_lib.ORB_E_INVALID, "local map: obs_start needs n_mp + 1 entries, kf_by_order n_kf and mp_track n_mp per frame")
        return LocalMapView(_addr(mp), _addr(view["obs_start"]), _addr(view["obs"]), _addr(view["kf"]), _addr(view["kf_mp"]),
                            _addr(view["children"]), _addr(view["kf_by_order"]), _addr(trk), n_mp, _nrec(view["obs"]), n_kf,
                            int(view["kf_mp"].shape[0]), int(view["children"].shape[0]), n_mp if batched else 0)

    def UpdateLocalMap(self, view, frames, vote_mp, n_vote, frame_mp, n_frame, cap_kf, cap_mp, dropped_mp=None, n_dropped=None, work=None,
                       out=None):
        """Tracking::UpdateLocalKeyFrames + UpdateLocalPoints + the marking loop of SearchLocalPoints for B frames (orbm_update_local_map),
        asynchronously on the inputs' stream.  view: see _local_map_view; frames: LOCALMAP_FRAME_DTYPE [B] (torch: uint8 [B, 8]); vote_mp /
        frame_mp: int32 [B, cap_f] map-point indices, in/out (bad points are nulled), the same array twice where the current frame votes;
        n_vote / n_frame int32 [B]; dropped_mp int32 [B, cap_dropped] with n_dropped [B], optional.  work: LocalMapWorkspace(view, B) of an
        earlier call; out: the dict of an earlier call to write into.
        -> dict(local_kf [B, cap_kf], n_local_kf, n_local_kf_required, ref_kf, max_votes [B], local_src [B, cap_mp], nmp, nmp_required [B],
        local_mp [B, cap_mp, 48] u8 view of MAP_POINT_DTYPE, track [B, cap_mp, 32] u8 view of TRACK_DTYPE, flags [B] of LM_* bits, work, cap_kf,
        cap_mp): local_mp, nmp and track are the mp, nmp and track of ProjectMapPoints(PROJ_LOCAL_MAP).  check_local_map() reports overflow."""
        B, like = vote_mp.shape[0], vote_mp
        if out is None:
            i32 = lambda *sh: zeros(like, sh, np.int32)   # noqa: E731
            out = dict(local_kf=i32(B, cap_kf), n_local_kf=i32(B), n_local_kf_required=i32(B), ref_kf=i32(B), max_votes=i32(B),
                       local_src=i32(B, cap_mp), nmp=i32(B), nmp_required=i32(B),
                       local_mp=zeros(like, (B, cap_mp, MAP_POINT_DTYPE.itemsize), np.uint8),
                       track=zeros(like, (B, cap_mp, TRACK_DTYPE.itemsize), np.uint8), flags=i32(B))
        out["work"] = work if work is not None else out.get("work")
        if out["work"] is None:
            out["work"] = self.LocalMapWorkspace(view, B)
        out["cap_kf"], out["cap_mp"] = int(cap_kf), int(cap_mp)
        V = self._local_map_view(view)
        if out["work"].shape[0] * 4 < self._L.orbm_local_map_workspace_bytes(V.n_kf, V.n_mp, B):
            raise OrbHipError(_lib.ORB_E_INVALID, "local map: the workspace is too small for this view and batch")
        L = LocalMapLists(_addr(vote_mp), _addr(n_vote), _addr(frame_mp), _addr(n_frame), _addr(dropped_mp), _addr(n_dropped),
                          vote_mp.shape[1], 0 if dropped_mp is None else dropped_mp.shape[1])
        if frame_mp.shape[1] != vote_mp.shape[1]:
            raise OrbHipError(_lib.ORB_E_INVALID, "local map: vote_mp and frame_mp share one cap_f")
        O = LocalMapOut(*[_addr(out[k]) for k in ("local_kf", "n_local_kf", "n_local_kf_required", "ref_kf", "max_votes", "local_src", "nmp",
                                                  "nmp_required", "local_mp", "track", "flags")], int(cap_kf), int(cap_mp))
        self._check(self._L.orbm_update_local_map(C.byref(V), ptr(frames), C.byref(L), B, C.byref(O), ptr(out["work"]), stream(like)))
        return out

    def check_local_map(self, local):
        """Host check (reads the counts and flags back): OrbHipError(ORB_E_INVALID) if a frame was flagged for an index out of range,
        OrbHipError(ORB_E_CAPACITY) if its key frames or points did not fit cap_kf / cap_mp."""
        fl = to_host(local["flags"])
        bad = np.nonzero(fl & LM_BAD_INDEX)[0]
        if len(bad):
            raise OrbHipError(_lib.ORB_E_INVALID, "local map: %d frame(s) flagged for a bad index (first: frame %d)" % (len(bad), bad[0]))
        rk, rp = to_host(local["n_local_kf_required"]), to_host(local["nmp_required"])
        over = np.nonzero((rk > local["cap_kf"]) | (rp > local["cap_mp"]))[0]
        check_capacity(over, lambda b: "local map: %d frame(s) need more than cap_kf = %d key frames or cap_mp = %d points (frame %d: %d, %d)"
                       % (len(over), local["cap_kf"], local["cap_mp"], b, int(rk[b]), int(rp[b])))

    def StoreLocalTracks(self, local, view, track=None):
        """The scatter-back after ProjectMapPoints (orbm_store_local_tracks): the track entries of the local points (track: default
        local["track"], which the projection updated in place) go back to view["mp_track"], so that the next frame reads them."""
        V = self._local_map_view(view)
        trk = local["track"] if track is None else track
        self._check(self._L.orbm_store_local_tracks(ptr(trk), ptr(local["local_src"]), ptr(local["nmp"]), local["cap_mp"],
                                                    local["local_src"].shape[0], ptr(view["mp_track"]), V.track_stride, V.n_mp, stream(trk)))

    # -- key-frame culling (include/orbhip.h "Key-frame culling"): LocalMapping::KeyFrameCulling on the device map
    @staticmethod
    def _cull_view(view):
        """orbm_localmap_view of the members the culling reads: mp, obs_start, obs, kf, kf_mp of the dict _local_map_view takes"""
        n_mp, n_kf = _nrec(view["mp"]), _nrec(view["kf"])
        if view["obs_start"].shape[0] != n_mp + 1:
            raise OrbHipError(_lib.ORB_E_INVALID, "key-frame culling: obs_start needs n_mp + 1 entries")
        return LocalMapView(_addr(view["mp"]), _addr(view["obs_start"]), _addr(view["obs"]), _addr(view["kf"]), _addr(view["kf_mp"]), None,
                            None, None, n_mp, _nrec(view["obs"]), n_kf, int(view["kf_mp"].shape[0]), 0, 0)

    @staticmethod
    def _cull_in(view, cull, problems=None, candidates=None, n_cand_max=0):
        """orbm_cull_in of cull = dict(ckf CULL_KEYFRAME_DTYPE [n_kf], feat uint8 [rows][, mp_nobs int32 [n_mp]])"""
        if _nrec(cull["ckf"]) != _nrec(view["kf"]) or cull["feat"].shape[0] != view["kf_mp"].shape[0] or \
                (cull.get("mp_nobs") is not None and cull["mp_nobs"].shape[0] != _nrec(view["mp"])):
            raise OrbHipError(_lib.ORB_E_INVALID, "key-frame culling: ckf is parallel to kf, feat to kf_mp and mp_nobs to mp")
        return CullIn(_addr(cull["ckf"]), _addr(cull["feat"]), _addr(cull.get("mp_nobs")), _addr(problems), _addr(candidates),
                      0 if candidates is None else int(candidates.shape[0]), int(n_cand_max))

    def CullWorkspace(self, view, batch):
        """uint8 workspace of CullKeyFrames / ApplyKeyFrameCulling for the view's sizes, allocated like the view's arrays"""
        n = self._L.orbm_cull_workspace_bytes(_nrec(view["kf"]), _nrec(view["mp"]), _nrec(view["obs"]), int(batch))
        return zeros(view["obs_start"], (max(n, 16),), np.uint8)

    def CullKeyFrames(self, view, cull, problems, candidates, cap_cand, n_cand_max=None, work=None, out=None):
        """LocalMapping::KeyFrameCulling (LocalMapping.cc:1176-1321) for B independent problems on one view (orbm_cull_keyframes),
        asynchronously on the inputs' stream; the map is not changed (ApplyKeyFrameCulling folds one problem's outcome in).
        view: the dict UpdateLocalMap takes (mp, obs_start, obs, kf, kf_mp are read); cull: dict(ckf, feat[, mp_nobs]) as
        flatten_cull_keyframes builds them; problems: CULL_PROBLEM_DTYPE [B] (torch: uint8 [B, 24]); candidates: int32, shared;
        n_cand_max: the greatest n_cand of the problems (default: cap_cand); work: CullWorkspace(view, B).
        -> dict(code [B, cap_cand] u8 of CULL_CODE_*, nmps / nred [B, cap_cand], events [B, cap_cand, 12] u8 view of CULL_EVENT_DTYPE, n_events [B],
        flags [B] of CULL_BAD_INDEX | CULL_UNSUPPORTED, work, batch).  check_cull_flags() reads the flags back."""
        B, like = _nrec(problems), candidates
        if out is None:
            i32 = lambda *sh: zeros(like, sh, np.int32)   # noqa: E731
            out = dict(code=zeros(like, (B, cap_cand), np.uint8), nmps=i32(B, cap_cand), nred=i32(B, cap_cand),
                       events=zeros(like, (B, cap_cand, CULL_EVENT_DTYPE.itemsize), np.uint8), n_events=i32(B), flags=i32(B))
        out["work"] = work if work is not None else out.get("work")
        if out["work"] is None:
            out["work"] = self.CullWorkspace(view, B)
        out["batch"] = B
        V = self._cull_view(view)
        if out["work"].shape[0] < self._L.orbm_cull_workspace_bytes(V.n_kf, V.n_mp, V.n_obs, B):
            raise OrbHipError(_lib.ORB_E_INVALID, "key-frame culling: the workspace is too small for this view and batch")
        I = self._cull_in(view, cull, problems, candidates, cap_cand if n_cand_max is None else n_cand_max)
        O = CullOut(*[_addr(out[k]) for k in ("code", "nmps", "nred", "events", "n_events", "flags")], int(cap_cand), 0)
        self._check(self._L.orbm_cull_keyframes(C.byref(V), C.byref(I), B, C.byref(O), ptr(out["work"]), stream(like)))
        return out

    def check_cull_flags(self, culled):
        """Host check (reads the flag words back): OrbHipError(ORB_E_INVALID) if a problem met an index out of range or a rig record."""
        fl = to_host(culled["flags"])
        bad = np.nonzero(fl & (CULL_BAD_INDEX | CULL_UNSUPPORTED))[0]
        if len(bad):
            raise OrbHipError(_lib.ORB_E_INVALID, "key-frame culling: %d problem(s) flagged (problem %d: flags %d)"
                              % (len(bad), bad[0], int(fl[bad[0]])))

    def CullState(self, view, culled, problem=0):
        """Host copies of one problem's final state in the workspace: dict(nobs int32 [n_mp], rec uint8 [n_obs] of CULL_REC_*, mp_bad uint8
        [n_mp], kf_erased uint8 [n_kf], prev / next int32 [n_kf]).  Reads the workspace back."""
        n_kf, n_mp, n_obs = _nrec(view["kf"]), _nrec(view["mp"]), _nrec(view["obs"])
        Y = CullWorkspaceLayout()
        self._check(self._L.orbm_cull_workspace(n_kf, n_mp, n_obs, C.byref(Y)))
        w = to_host(culled["work"])[problem * Y.stride:(problem + 1) * Y.stride]
        sec = lambda off, n, dt: w[off:off + n * np.dtype(dt).itemsize].view(dt).copy()   # noqa: E731
        return dict(nobs=sec(Y.nobs, n_mp, np.int32), rec=(sec(Y.rec, n_obs, np.uint32) & 3).astype(np.uint8), mp_bad=sec(Y.mp_bad, n_mp, np.uint8),
                    kf_erased=sec(Y.kf_erased, n_kf, np.uint8), prev=sec(Y.prev, n_kf, np.int32), next=sec(Y.next, n_kf, np.int32))

    def ApplyKeyFrameCulling(self, view, cull, culled, ref, cap_obs_out, problem=0, out=None):
        """Folds problem `problem` of CullKeyFrames' outcome into the device map (orbm_apply_keyframe_culling), on the inputs' stream: the flags
        of view["mp"] and view["kf"], view["kf_mp"], cull["ckf"] links, cull["mp_nobs"] when given and ref (REFRESH_POINT_DTYPE [n_mp]) are
        updated in place; the compacted observation CSR goes to new arrays.
        -> dict(obs_start int32 [n_mp + 1], obs [cap_obs_out, 12] u8 view of OBSERVATION_DTYPE, result int32 [2]: records needed, overflow).
        On overflow nothing is written; check_cull_applied() reports it."""
        V = self._cull_view(view)
        like = view["obs_start"]
        if ref.shape[0] != V.n_mp:
            raise OrbHipError(_lib.ORB_E_INVALID, "ApplyKeyFrameCulling: ref needs n_mp entries")
        if out is None:
            out = dict(obs_start=zeros(like, (V.n_mp + 1,), np.int32), obs=zeros(like, (max(cap_obs_out, 1), OBSERVATION_DTYPE.itemsize), np.uint8),
                       result=zeros(like, (2,), np.int32))
        out["cap_obs_out"] = int(cap_obs_out)
        I = self._cull_in(view, cull)
        Y = CullApply(_addr(view["mp"]), _addr(view["kf"]), _addr(cull["ckf"]), _addr(view["kf_mp"]), _addr(cull.get("mp_nobs")), _addr(ref),
                      _addr(out["obs_start"]), _addr(out["obs"]), _addr(out["result"]), int(cap_obs_out), 0)
        self._check(self._L.orbm_apply_keyframe_culling(C.byref(V), C.byref(I), culled["batch"], int(problem), C.byref(Y), ptr(culled["work"]),
                                                        stream(like)))
        return out

    def check_cull_applied(self, applied):
        """Host check: OrbHipError(ORB_E_CAPACITY) if the compacted CSR did not fit cap_obs_out (nothing was written then)."""
        r = to_host(applied["result"])
        check_capacity([0] if r[1] else [], lambda _: "apply culling: %d observation records do not fit cap_obs_out = %d"
                       % (int(r[0]), applied["cap_obs_out"]))
