"""The head of LocalMapping::Run on the device map (include/orbhip.h "New key frame"), above the C ABI: the association loop of
ProcessNewKeyFrame, MapPointCulling with the map effects of MapPoint::SetBadFlag, and mlpRecentAddedMapPoints.

Arrays may be torch CUDA tensors (product path) or numpy arrays (the emulated test build).  The caller runs ComputeBoW before
ProcessNewKeyFrame and CovisibilityGraph.UpdateConnections right after it, on the same stream."""
import ctypes as C

import numpy as np

from . import _lib
from ._abi import (MPCULL_MONOCULAR, NEWKF_BAD_INDEX, NEWKF_OBS_OVERFLOW, NEWKF_R_FLAGS, NEWKF_R_N_OBS, NEWKF_R_N_PUSH_REQUIRED,
                   NEWKF_R_WORDS, NEWKF_RECENT_OVERFLOW, NEWKF_REFRESH_OVERFLOW, NEWKF_UNSUPPORTED, OBSERVATION_DTYPE,
                   LocalMapView, MpCullOut, NewKfIn, NewKfOut, RefreshParams)
from ._lib import OrbHipError, check, ptr, stream, to_host, zeros
from .matcher import _addr, _nrec


class NewKeyFrame:
    """scale_factors: mvScaleFactors of the key frames (1..16 levels), as UpdateNormalAndDepth reads them.  cap_recent: the capacity of the
    recent list (every list array of a call has that many entries)."""

    def __init__(self, scale_factors, cap_recent, *, lib=None):
        self._L = lib if lib is not None else _lib.load()
        n = len(scale_factors)
        if not 1 <= n <= 16 or cap_recent < 1:
            raise OrbHipError(_lib.ORB_E_INVALID, "NewKeyFrame: 1..16 levels, cap_recent >= 1")
        P = RefreshParams()
        P.what, P.nlevels = 3, n
        P.scale_factors[:n] = [float(x) for x in scale_factors]
        self.params, self.cap_recent = P, int(cap_recent)

    @staticmethod
    def _view(view, by_order=True):
        n_mp, n_kf = _nrec(view["mp"]), _nrec(view["kf"])
        if view["obs_start"].shape[0] != n_mp + 1 or (by_order and view["kf_by_order"].shape[0] != n_kf):
            raise OrbHipError(_lib.ORB_E_INVALID, "NewKeyFrame: obs_start needs n_mp + 1 entries, kf_by_order n_kf")
        return LocalMapView(_addr(view["mp"]), _addr(view["obs_start"]), _addr(view["obs"]), _addr(view["kf"]), _addr(view["kf_mp"]), None,
                            _addr(view.get("kf_by_order")), None, n_mp, _nrec(view["obs"]), n_kf, int(view["kf_mp"].shape[0]), 0, 0)

    def _in(self, V, kfs, cap_feat):
        if _nrec(kfs["ckf"]) != V.n_kf or kfs["feat"].shape[0] != V.n_kf_mp_rows:
            raise OrbHipError(_lib.ORB_E_INVALID, "NewKeyFrame: ckf is parallel to kf, feat to kf_mp")
        for k in ("found", "visible", "first_kf_id", "mp_nobs", "ref"):
            if kfs.get(k) is not None and kfs[k].shape[0] != V.n_mp:
                raise OrbHipError(_lib.ORB_E_INVALID, "NewKeyFrame: %s needs n_mp entries" % k)
        kd = kfs.get("kf_desc")
        return NewKfIn(_addr(kfs["ckf"]), _addr(kfs["feat"]), _addr(kfs.get("ref")), _addr(kfs.get("center")), _addr(kd), _addr(kfs.get("found")),
                       _addr(kfs.get("visible")), _addr(kfs.get("first_kf_id")), 0 if kd is None else int(kd.shape[0]), int(cap_feat))

    def Workspace(self, view, cap_feat):
        """uint8 workspace for the view's sizes (either call), allocated like the view's arrays"""
        n = self._L.orbm_newkf_workspace_bytes(_nrec(view["kf"]), _nrec(view["mp"]), int(cap_feat))
        if n == 0:
            raise OrbHipError(_lib.ORB_E_INVALID, "NewKeyFrame: cap_feat below 1")
        return zeros(view["obs_start"], (n,), np.uint8)

    def _work(self, view, cap_feat, work):
        if work is None:
            return self.Workspace(view, cap_feat)
        if work.shape[0] < self._L.orbm_newkf_workspace_bytes(_nrec(view["kf"]), _nrec(view["mp"]), int(cap_feat)):
            raise OrbHipError(_lib.ORB_E_INVALID, "NewKeyFrame: the workspace is too small for this view")
        return work

    def ProcessNewKeyFrame(self, view, kfs, current_kf, cap_feat, cap_obs_out, recent, n_recent, work=None, out=None):
        """The association loop of LocalMapping::ProcessNewKeyFrame for key frame current_kf (orbm_process_new_keyframe), asynchronously on the
        inputs' stream.  view: the dict UpdateLocalMap takes (mp, obs_start, obs, kf, kf_mp, kf_by_order); view["mp"] is updated in place.
        kfs: dict(ckf CULL_KEYFRAME_DTYPE [n_kf], feat uint8 [rows], ref REFRESH_POINT_DTYPE [n_mp], center KEYFRAME_CENTER_DTYPE [n_kf],
        kf_desc uint8 [rows_d, 32], mp_desc uint8 [n_desc_rows, 32] (rewritten for the points that gained a record)[, mp_nobs int32 [n_mp],
        in/out]).  recent int32 [cap_recent], n_recent int32 [1]: the recent list, in/out.
        -> dict(code uint8 [cap_feat], sel [cap_feat], obs_start [n_mp + 1], obs [cap_obs_out, 12] u8 view of OBSERVATION_DTYPE,
        result [NEWKF_R_WORDS], work).  check_flags() reads the result words back."""
        V, like = self._view(view), view["obs_start"]
        I = self._in(V, kfs, cap_feat)
        if recent.shape[0] != self.cap_recent:
            raise OrbHipError(_lib.ORB_E_INVALID, "NewKeyFrame: the recent list has cap_recent entries")
        if out is None:
            out = dict(code=zeros(like, (cap_feat,), np.uint8), sel=zeros(like, (cap_feat,), np.int32), obs_start=zeros(like, (V.n_mp + 1,), np.int32),
                       obs=zeros(like, (max(cap_obs_out, 1), OBSERVATION_DTYPE.itemsize), np.uint8), result=zeros(like, (NEWKF_R_WORDS,), np.int32))
        out["work"] = self._work(view, cap_feat, work if work is not None else out.get("work"))
        out["caps"] = dict(cap_obs_out=int(cap_obs_out), cap_recent=self.cap_recent)
        O = NewKfOut(_addr(view["mp"]), _addr(kfs.get("mp_nobs")), _addr(kfs["mp_desc"]), _addr(out["code"]), _addr(out["sel"]),
                     _addr(out["obs_start"]), _addr(out["obs"]), _addr(recent), _addr(n_recent), _addr(out["result"]),
                     int(kfs["mp_desc"].shape[0]), int(cap_obs_out), self.cap_recent, 0)
        check(self._L.orbm_process_new_keyframe(C.byref(V), C.byref(I), int(current_kf), C.byref(self.params), C.byref(O), ptr(out["work"]),
                                                stream(like)), "orbm_process_new_keyframe")
        return out

    def PushRecent(self, sel, recent, n_recent, out=None):
        """mlpRecentAddedMapPoints.push_back of the points AppendNewMapPoints made (orbm_recent_points_push): the entries >= 0 of sel, in
        order.  -> dict(result [NEWKF_R_WORDS])"""
        if out is None:
            out = dict(result=zeros(sel, (NEWKF_R_WORDS,), np.int32))
        out["caps"] = dict(cap_obs_out=0, cap_recent=self.cap_recent)
        check(self._L.orbm_recent_points_push(ptr(sel), int(sel.shape[0]), ptr(recent), ptr(n_recent), self.cap_recent, ptr(out["result"]),
                                              stream(sel)), "orbm_recent_points_push")
        return out

    def MapPointCulling(self, view, kfs, current_kf, recent, n_recent, cap_obs_out, bMonocular=False, work=None, out=None):
        """LocalMapping::MapPointCulling over the recent list (orbm_cull_map_points), asynchronously on the inputs' stream.  view: mp,
        obs_start, obs, kf, kf_mp; view["mp"] flags and view["kf_mp"] are updated in place.  kfs: dict(ckf, feat, found, visible int32 [n_mp],
        first_kf_id uint32-as-int32 [n_mp][, mp_nobs int32 [n_mp]]).
        -> dict(code uint8 [cap_recent], recent [cap_recent], n_recent [1] (the surviving list: the next call's input), culled [cap_recent],
        n_culled [1], obs_start [n_mp + 1], obs [cap_obs_out, 12], result [NEWKF_R_WORDS], work)."""
        V, like = self._view(view, by_order=False), view["obs_start"]
        I = self._in(V, kfs, 1)
        cap = self.cap_recent
        if recent.shape[0] != cap:
            raise OrbHipError(_lib.ORB_E_INVALID, "NewKeyFrame: the recent list has cap_recent entries")
        if out is None:
            i32 = lambda *sh: zeros(like, sh, np.int32)   # noqa: E731
            out = dict(code=zeros(like, (cap,), np.uint8), recent=i32(cap), n_recent=i32(1), culled=i32(cap), n_culled=i32(1),
                       obs_start=i32(V.n_mp + 1), obs=zeros(like, (max(cap_obs_out, 1), OBSERVATION_DTYPE.itemsize), np.uint8),
                       result=i32(NEWKF_R_WORDS))
        out["work"] = self._work(view, 1, work if work is not None else out.get("work"))
        out["caps"] = dict(cap_obs_out=int(cap_obs_out), cap_recent=cap)
        O = MpCullOut(_addr(view["mp"]), _addr(view["kf_mp"]), _addr(out["code"]), _addr(out["recent"]), _addr(out["n_recent"]),
                      _addr(out["culled"]), _addr(out["n_culled"]), _addr(out["obs_start"]), _addr(out["obs"]), _addr(out["result"]),
                      int(cap_obs_out), cap)
        check(self._L.orbm_cull_map_points(C.byref(V), C.byref(I), ptr(kfs.get("mp_nobs")), int(current_kf),
                                           MPCULL_MONOCULAR if bMonocular else 0, ptr(recent), ptr(n_recent), C.byref(O), ptr(out["work"]),
                                           stream(like)), "orbm_cull_map_points")
        return out

    def check_flags(self, out):
        """Host check (reads the result words back): OrbHipError(ORB_E_INVALID) for a bad index or a rig record, OrbHipError(ORB_E_CAPACITY)
        for a capacity that did not hold.  ORBM_NEWKF_UNSORTED is not an error: the rows were copied as they lay."""
        r, caps = to_host(out["result"]), out["caps"]
        fl = int(r[NEWKF_R_FLAGS])
        if fl & (NEWKF_BAD_INDEX | NEWKF_UNSUPPORTED):
            raise OrbHipError(_lib.ORB_E_INVALID, "NewKeyFrame: a bad index or a rig record was met and treated as absent (flags %d)" % fl)
        if fl & NEWKF_OBS_OVERFLOW:
            raise OrbHipError(_lib.ORB_E_CAPACITY, "NewKeyFrame: %d observation records do not fit the capacity of %d; nothing was written"
                              % (int(r[NEWKF_R_N_OBS]), caps["cap_obs_out"]))
        if fl & NEWKF_RECENT_OVERFLOW:
            raise OrbHipError(_lib.ORB_E_CAPACITY, "NewKeyFrame: %d pushes do not fit the recent list of %d"
                              % (int(r[NEWKF_R_N_PUSH_REQUIRED]), caps["cap_recent"]))
        if fl & NEWKF_REFRESH_OVERFLOW:
            raise OrbHipError(_lib.ORB_E_CAPACITY, "NewKeyFrame: a point has more usable records than ORBM_REFRESH_MAX_OBS")
