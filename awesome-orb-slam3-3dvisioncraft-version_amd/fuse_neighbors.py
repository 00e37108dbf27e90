"""LocalMapping::SearchInNeighbors on the device map (include/orbhip.h "Fusion in the neighbours"), above the C ABI: target selection, one
ORBmatcher::Fuse per target, the candidates and the Fuse into the current key frame, with MapPoint::Replace / AddObservation folded into the
map where it lies.

Arrays may be torch CUDA tensors (product path) or numpy arrays (the emulated test build).  The caller runs the tail of the reference
function right after, on the same stream: ORBmatcher.RefreshMapPoints over out["sel"] and CovisibilityGraph.UpdateConnections."""
import ctypes as C

import numpy as np

from . import _lib
from ._abi import (FUSENB_ABORT_BA, FUSENB_BAD_INDEX, FUSENB_CANDIDATE_OVERFLOW, FUSENB_EVENT_DTYPE, FUSENB_EVENT_OVERFLOW,  # noqa: F401
                   FUSENB_INERTIAL, FUSENB_MONOCULAR, FUSENB_OBS_OVERFLOW, FUSENB_POSE_DTYPE, FUSENB_R_FLAGS, FUSENB_R_N_CANDIDATES_REQUIRED,
                   FUSENB_R_N_EVENTS, FUSENB_R_N_OBS, FUSENB_R_N_TARGETS_REQUIRED, FUSENB_R_WORDS, FUSENB_REFRESH_OVERFLOW,
                   FUSENB_TARGET_OVERFLOW, FUSENB_UNSORTED, FUSENB_UNSUPPORTED, OBSERVATION_DTYPE, FuseNbIn, FuseNbOut, FuseNbParams, GridParams,
                   LocalMapView)
from ._lib import OrbHipError, check, ptr, stream, to_host, zeros
from .matcher import _addr, _nrec


def flatten_fuse_poses(keyframes):
    """keyframes: the list flatten_local_map_keyframes takes, every dict with Rcw (3x3), tcw (3), Ow (3) as the reference's getters give them
    -> FUSENB_POSE_DTYPE [n]"""
    pose = np.zeros(len(keyframes), FUSENB_POSE_DTYPE)
    for i, k in enumerate(keyframes):
        if k is not None:
            pose[i]["Rcw"] = np.asarray(k["Rcw"], np.float32).reshape(9)
            pose[i]["tcw"], pose[i]["Ow"] = np.asarray(k["tcw"], np.float32), np.asarray(k["Ow"], np.float32)
    return pose


class NeighborFusion:
    """One camera and one extractor setting: K = (fx, fy, cx, cy), mbf, bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY), grid = (mnMinX, mnMinY,
    mfGridElementWidthInv, mfGridElementHeightInv), mvScaleFactors, mvInvLevelSigma2, mfLogScaleFactor."""

    def __init__(self, K, mbf, bounds, grid, scale_factors, inv_level_sigma2, log_scale_factor, th=3.0, *, lib=None):
        self._L = lib if lib is not None else _lib.load()
        n = len(scale_factors)
        if not 1 <= n <= 16 or len(inv_level_sigma2) != n:
            raise OrbHipError(_lib.ORB_E_INVALID, "SearchInNeighbors: 1..16 levels, one inverse sigma2 per level")
        P = FuseNbParams()
        P.fx, P.fy, P.cx, P.cy = [float(x) for x in K]
        P.mbf, P.th, P.nlevels = float(mbf), float(th), n
        P.bounds[:] = [float(x) for x in bounds]
        P.grid = GridParams(*[float(x) for x in grid])
        P.scale_factors[:n] = [float(x) for x in scale_factors]
        P.inv_level_sigma2[:n] = [float(x) for x in inv_level_sigma2]
        th_ = (C.c_float * 16)()
        check(self._L.orbm_predict_scale_thresholds(float(log_scale_factor), n, th_), "orbm_predict_scale_thresholds")
        P.level_thresholds[:] = list(th_)
        self.params = P

    @staticmethod
    def _view(view):
        n_mp, n_kf = _nrec(view["mp"]), _nrec(view["kf"])
        if view["obs_start"].shape[0] != n_mp + 1 or view["kf_by_order"].shape[0] != n_kf:
            raise OrbHipError(_lib.ORB_E_INVALID, "SearchInNeighbors: obs_start needs n_mp + 1 entries, kf_by_order n_kf")
        return LocalMapView(_addr(view["mp"]), _addr(view["obs_start"]), _addr(view["obs"]), _addr(view["kf"]), _addr(view["kf_mp"]), None,
                            _addr(view["kf_by_order"]), None, n_mp, _nrec(view["obs"]), n_kf, int(view["kf_mp"].shape[0]), 0, 0)

    def Workspace(self, view, cap_feat, cap_candidates, cap_events):
        """uint8 workspace for the view's sizes and these capacities, allocated like the view's arrays"""
        n = self._L.orbm_fusenb_workspace_bytes(_nrec(view["kf"]), _nrec(view["mp"]), _nrec(view["obs"]), int(cap_feat), int(cap_candidates),
                                                int(cap_events))
        if n == 0:
            raise OrbHipError(_lib.ORB_E_INVALID, "SearchInNeighbors: capacities below 1, or cap_feat above 65535")
        return zeros(view["obs_start"], (n,), np.uint8)

    def SearchInNeighbors(self, view, fuse, current_kf, cap_feat, cap_targets, cap_candidates, cap_events, cap_obs_out, bMonocular=False,
                          bInertial=False, bAbortBA=False, work=None, out=None):
        """LocalMapping::SearchInNeighbors for key frame current_kf (orbm_search_in_neighbors), asynchronously on the inputs' stream.
        view: the dict UpdateLocalMap takes (mp, obs_start, obs, kf, kf_mp, kf_by_order); view["mp"] flags and view["kf_mp"] are updated in place.
        fuse: dict(ckf CULL_KEYFRAME_DTYPE [n_kf], pose FUSENB_POSE_DTYPE [n_kf], feat uint8 [rows], kps KP_DTYPE [rows], u_right float32 [rows],
        kf_desc uint8 [rows_d, 32], ordered_kf int32 [n_kf, cap_conn], n_ordered int32 [n_kf], mp_desc uint8 [n_desc_rows, 32] (the survivors'
        rows are rewritten), fuse_target uint32-as-int32 [n_kf] (mnFuseTargetForKF, in/out)[, mp_nobs, found, visible int32 [n_mp], in/out]).
        -> dict(targets [cap_targets], candidates [cap_candidates], nfused [cap_targets + 1], events [cap_events, 32] u8 view of
        FUSENB_EVENT_DTYPE, replaced [n_mp], sel [cap_feat], obs_start [n_mp + 1], obs [cap_obs_out, 12] u8 view of OBSERVATION_DTYPE,
        result [FUSENB_R_WORDS], work).  check_flags() reads the result words back."""
        V, like = self._view(view), view["obs_start"]
        if _nrec(fuse["ckf"]) != V.n_kf or _nrec(fuse["pose"]) != V.n_kf or fuse["feat"].shape[0] != V.n_kf_mp_rows or \
                _nrec(fuse["kps"]) != V.n_kf_mp_rows or fuse["u_right"].shape[0] != V.n_kf_mp_rows or fuse["ordered_kf"].shape[0] != V.n_kf or \
                fuse["n_ordered"].shape[0] != V.n_kf or fuse["fuse_target"].shape[0] != V.n_kf:
            raise OrbHipError(_lib.ORB_E_INVALID, "SearchInNeighbors: ckf, pose, the ordered rows and fuse_target are parallel to kf; feat, kps "
                                                  "and u_right to kf_mp")
        for k in ("mp_nobs", "found", "visible"):
            if fuse.get(k) is not None and fuse[k].shape[0] != V.n_mp:
                raise OrbHipError(_lib.ORB_E_INVALID, "SearchInNeighbors: %s needs n_mp entries" % k)
        if out is None:
            i32 = lambda *sh: zeros(like, sh, np.int32)   # noqa: E731
            out = dict(targets=i32(cap_targets), candidates=i32(cap_candidates), nfused=i32(cap_targets + 1),
                       events=zeros(like, (cap_events, FUSENB_EVENT_DTYPE.itemsize), np.uint8), replaced=i32(max(V.n_mp, 1)),
                       sel=i32(cap_feat), obs_start=i32(V.n_mp + 1), obs=zeros(like, (max(cap_obs_out, 1), OBSERVATION_DTYPE.itemsize), np.uint8),
                       result=i32(FUSENB_R_WORDS))
        out["work"] = work if work is not None else out.get("work")
        if out["work"] is None:
            out["work"] = self.Workspace(view, cap_feat, cap_candidates, cap_events)
        if out["work"].shape[0] < self._L.orbm_fusenb_workspace_bytes(V.n_kf, V.n_mp, V.n_obs, int(cap_feat), int(cap_candidates), int(cap_events)):
            raise OrbHipError(_lib.ORB_E_INVALID, "SearchInNeighbors: the workspace is too small for this view and these capacities")
        out["caps"] = dict(cap_targets=int(cap_targets), cap_candidates=int(cap_candidates), cap_events=int(cap_events),
                           cap_obs_out=int(cap_obs_out))
        I = FuseNbIn(_addr(fuse["ckf"]), _addr(fuse["pose"]), _addr(fuse["feat"]), _addr(fuse["kps"]), _addr(fuse["u_right"]),
                     _addr(fuse["kf_desc"]), _addr(fuse["ordered_kf"]), _addr(fuse["n_ordered"]), _addr(fuse.get("mp_nobs")),
                     int(fuse["kf_desc"].shape[0]), int(fuse["ordered_kf"].shape[1]), int(cap_feat), 0)
        O = FuseNbOut(_addr(view["mp"]), _addr(view["kf_mp"]), _addr(fuse.get("mp_nobs")), _addr(fuse.get("found")), _addr(fuse.get("visible")),
                      _addr(fuse["mp_desc"]), _addr(fuse["fuse_target"]), _addr(out["targets"]), _addr(out["candidates"]), _addr(out["nfused"]),
                      _addr(out["events"]), _addr(out["replaced"]), _addr(out["sel"]), _addr(out["obs_start"]), _addr(out["obs"]),
                      _addr(out["result"]), int(fuse["mp_desc"].shape[0]), int(cap_targets), int(cap_candidates), int(cap_events),
                      int(cap_obs_out), 0)
        P = FuseNbParams.from_buffer_copy(self.params)
        P.current_kf = int(current_kf)
        P.flags = (FUSENB_MONOCULAR if bMonocular else 0) | (FUSENB_INERTIAL if bInertial else 0) | (FUSENB_ABORT_BA if bAbortBA else 0)
        check(self._L.orbm_search_in_neighbors(C.byref(V), C.byref(I), C.byref(P), C.byref(O), ptr(out["work"]), stream(like)),
              "orbm_search_in_neighbors")
        return out

    def check_flags(self, out):
        """Host check (reads the result words back): OrbHipError(ORB_E_INVALID) for a bad index or a rig record, OrbHipError(ORB_E_CAPACITY)
        for any capacity that did not hold.  ORBM_FUSENB_UNSORTED is not an error: the rows were sorted."""
        r, caps = to_host(out["result"]), out["caps"]
        fl = int(r[FUSENB_R_FLAGS])
        if fl & (FUSENB_BAD_INDEX | FUSENB_UNSUPPORTED):
            raise OrbHipError(_lib.ORB_E_INVALID, "SearchInNeighbors: a bad index or a rig record was met and treated as absent (flags %d)" % fl)
        for bit, what, need, cap in ((FUSENB_TARGET_OVERFLOW, "targets", r[FUSENB_R_N_TARGETS_REQUIRED], caps["cap_targets"]),
                                     (FUSENB_CANDIDATE_OVERFLOW, "candidates", r[FUSENB_R_N_CANDIDATES_REQUIRED], caps["cap_candidates"]),
                                     (FUSENB_EVENT_OVERFLOW, "events", r[FUSENB_R_N_EVENTS] + 1, caps["cap_events"]),
                                     (FUSENB_OBS_OVERFLOW, "observation records", r[FUSENB_R_N_OBS], caps["cap_obs_out"])):
            if fl & bit:
                raise OrbHipError(_lib.ORB_E_CAPACITY, "SearchInNeighbors: %d %s do not fit the capacity of %d" % (int(need), what, cap))
        if fl & FUSENB_REFRESH_OVERFLOW:
            raise OrbHipError(_lib.ORB_E_CAPACITY, "SearchInNeighbors: a merged point has more usable records than ORBM_REFRESH_MAX_OBS")
