"""Optimizer::LocalBundleAdjustment on the device map (include/orbhip.h "Local bundle adjustment on the device map"), above the C ABI: the
window build (selection and flattening), the solver as it is, and the write-back (outlier pass, erase loop, poses, points, normals).

Arrays may be torch CUDA tensors (product path) or numpy arrays (the emulated test build).  The step sits between SearchInNeighbors and
KeyFrameCulling on the same stream; the out-CSR of Apply is the next step's view."""
import ctypes as C

import numpy as np

from . import _lib
from ._abi import (CAM_DTYPE, EDGE_DTYPE, LBA_A_FLAGS, LBA_A_N_ERASED, LBA_A_N_WENT_BAD, LBA_A_WORDS, LBA_BAD_INDEX, LBA_EARLY_RETURN,
                   LBA_OVERFLOW, LBA_R_FLAGS, LBA_R_N_EDGES, LBA_R_N_EDGES_REQUIRED, LBA_R_N_POINTS_REQUIRED, LBA_R_N_POSES_REQUIRED,
                   LBA_R_NUM_FIXED_KF, LBA_R_WORDS, LBA_UNSUPPORTED, OBSERVATION_DTYPE, LbaApply, LbaIn, LbaProblem, LbaSystem, LbaWindow,
                   LocalMapView)
from ._lib import OrbHipError, check, ptr, stream, to_host, zeros
from .lba import HUBER_MONO, HUBER_STEREO
from .matcher import _addr, _nrec


class LocalBA:
    """inv_level_sigma2 / scale_factors: mvInvLevelSigma2 / mvScaleFactors of the key frames (1..16 levels).  camera: one CAM_DTYPE record
    (pinhole) for every key frame.  cap_p / cap_l / cap_e: the window slabs' capacities in poses, points and edges."""

    def __init__(self, inv_level_sigma2, scale_factors, camera, cap_p, cap_l, cap_e, *, lib=None, huber=(HUBER_MONO, HUBER_STEREO)):
        self._L = lib if lib is not None else _lib.load()
        n = len(inv_level_sigma2)
        if not 1 <= n <= 16 or len(scale_factors) != n or min(cap_p, cap_l, cap_e) < 1:
            raise OrbHipError(_lib.ORB_E_INVALID, "LocalBA: 1..16 levels, capacities >= 1")
        self.nlevels, self.caps, self.huber = n, (int(cap_p), int(cap_l), int(cap_e)), huber
        self.inv_level_sigma2 = [float(x) for x in inv_level_sigma2]
        self.scale_factors = [float(x) for x in scale_factors]
        self.camera = np.ascontiguousarray(np.asarray(camera, CAM_DTYPE).reshape(1))
        self._lm_ws = self._d_cam = None

    @staticmethod
    def _view(view):
        n_mp, n_kf = _nrec(view["mp"]), _nrec(view["kf"])
        if view["obs_start"].shape[0] != n_mp + 1:
            raise OrbHipError(_lib.ORB_E_INVALID, "LocalBA: obs_start needs n_mp + 1 entries")
        return LocalMapView(_addr(view["mp"]), _addr(view["obs_start"]), _addr(view["obs"]), _addr(view["kf"]), _addr(view["kf_mp"]), None,
                            None, None, n_mp, _nrec(view["obs"]), n_kf, int(view["kf_mp"].shape[0]), 0, 0)

    def _in(self, V, kfs):
        if _nrec(kfs["ckf"]) != V.n_kf or _nrec(kfs["pose"]) != V.n_kf or kfs["u_right"].shape[0] != V.n_kf_mp_rows or \
                _nrec(kfs["kps"]) != V.n_kf_mp_rows or kfs["n_ordered"].shape[0] != V.n_kf:
            raise OrbHipError(_lib.ORB_E_INVALID, "LocalBA: ckf, pose and the ordered rows are parallel to kf; kps and u_right to kf_mp")
        cap_conn = int(kfs["ordered_kf"].shape[1]) if V.n_kf else 1
        I = LbaIn(_addr(kfs["ckf"]), _addr(kfs["pose"]), _addr(kfs["kps"]), _addr(kfs["u_right"]), _addr(kfs["ordered_kf"]),
                  _addr(kfs["n_ordered"]), _addr(kfs.get("map")), cap_conn, self.nlevels)
        I.inv_level_sigma2[:self.nlevels] = self.inv_level_sigma2
        I.scale_factors[:self.nlevels] = self.scale_factors
        return I

    def _workspace_bytes(self, V, cap_conn):
        return self._L.orbm_lba_workspace_bytes(V.n_kf, V.n_mp, V.n_obs, V.n_kf_mp_rows, cap_conn, *self.caps)

    def Workspace(self, view, kfs):
        """uint8 workspace for the view's sizes (either call), allocated like the view's arrays"""
        V = self._view(view)
        n = self._workspace_bytes(V, int(kfs["ordered_kf"].shape[1]) if V.n_kf else 1)
        if n == 0:
            raise OrbHipError(_lib.ORB_E_INVALID, "LocalBA: a size is out of range")
        return zeros(view["obs_start"], (n,), np.uint8)

    def _work(self, view, kfs, V, I, work):
        if work is None:
            return self.Workspace(view, kfs)
        if work.shape[0] < self._workspace_bytes(V, I.cap_conn):
            raise OrbHipError(_lib.ORB_E_INVALID, "LocalBA: the workspace is too small for this view")
        return work

    def Window(self, like):
        """the slabs of one window, allocated like `like`: the arrays of an lba_problem of batch 1 and the ties to the map"""
        cap_p, cap_l, cap_e = self.caps
        i32, f64 = (lambda *sh: zeros(like, sh, np.int32)), (lambda *sh: zeros(like, sh, np.float64))
        return dict(poses=f64(cap_p, 7), pose_hidx=i32(cap_p), points=f64(cap_l, 3), edges=zeros(like, (cap_e, EDGE_DTYPE.itemsize), np.uint8),
                    lm_start=i32(cap_l + 1), pose_start=i32(cap_p + 1), pose_edges=i32(cap_e), n_poses=i32(1), n_points=i32(1), n_edges=i32(1),
                    pose_kf=i32(cap_p), pose_local=i32(cap_p), point_mp=i32(cap_l), edge_rec=i32(cap_e), result=i32(LBA_R_WORDS),
                    chi2=f64(cap_e), depth=f64(cap_e))

    def _window(self, w):
        return LbaWindow(*[_addr(w[k]) for k in ("poses", "pose_hidx", "points", "edges", "lm_start", "pose_start", "pose_edges", "n_poses",
                                                 "n_points", "n_edges", "pose_kf", "pose_local", "point_mp", "edge_rec", "result")], *self.caps, 0)

    def Build(self, view, kfs, current_kf, init_kf_id, win=None, work=None):
        """The window of key frame current_kf (orbm_lba_window_build), asynchronously on the inputs' stream.  view: mp, obs_start, obs, kf,
        kf_mp.  kfs: dict(ckf CULL_KEYFRAME_DTYPE [n_kf], pose FUSENB_POSE_DTYPE [n_kf], kps KP_DTYPE [rows], u_right float32 [rows],
        ordered_kf int32 [n_kf, cap_conn], n_ordered int32 [n_kf][, map COVIS_KEYFRAME_DTYPE [n_kf]]).
        -> the window dict (Window()) with "work".  check_build() reads the result words back."""
        V = self._view(view)
        I = self._in(V, kfs)
        win = win if win is not None else self.Window(view["obs_start"])
        win["work"] = self._work(view, kfs, V, I, work if work is not None else win.get("work"))
        O = self._window(win)
        check(self._L.orbm_lba_window_build(C.byref(V), C.byref(I), int(current_kf), int(init_kf_id) & 0xFFFFFFFF, C.byref(O), ptr(win["work"]),
                                            stream(view["obs_start"])), "orbm_lba_window_build")
        return win

    def check_build(self, win):
        """Host check (reads the result words back) -> the result words.  OrbHipError(ORB_E_INVALID) for a bad index or a rig record,
        OrbHipError(ORB_E_CAPACITY) where the window did not fit its slabs (nothing was written)."""
        r = to_host(win["result"])
        fl = int(r[LBA_R_FLAGS])
        if fl & LBA_OVERFLOW:
            raise OrbHipError(_lib.ORB_E_CAPACITY, "LocalBA: the window needs %d poses, %d points, %d edges; the slabs hold %d, %d, %d"
                              % ((int(r[LBA_R_N_POSES_REQUIRED]), int(r[LBA_R_N_POINTS_REQUIRED]), int(r[LBA_R_N_EDGES_REQUIRED])) + self.caps))
        if fl & (LBA_BAD_INDEX | LBA_UNSUPPORTED):
            raise OrbHipError(_lib.ORB_E_INVALID, "LocalBA: a bad index or a rig record was met and treated as absent (flags %d)" % fl)
        return r

    def _problem(self, win):
        like = win["poses"]
        if self._d_cam is None:
            cam = self.camera.view(np.uint8)
            if isinstance(like, np.ndarray):
                self._d_cam = cam
            else:
                import torch
                self._d_cam = torch.from_numpy(cam).to(like.device)
        P = LbaProblem(*[ptr(win[k]).value for k in ("poses", "pose_hidx", "points", "edges", "lm_start", "pose_start", "pose_edges")],
                       ptr(self._d_cam).value, *[ptr(win[k]).value for k in ("n_poses", "n_points", "n_edges")], *self.caps, 1,
                       self.huber[0], self.huber[1])
        if self._lm_ws is None:
            self._lm_ws = zeros(like, (self._L.lba_lm_workspace_bytes(C.byref(P), 1),), np.uint8)
        return P

    def Optimize(self, win, iterations, stop_flag=None):
        """optimizer.optimize(iterations) on the window (lba_optimize_stopflag; synchronous).  stop_flag: a host uint8 [1] array, or None.
        -> stats [4]"""
        P = self._problem(win)
        stats = np.zeros((1, 4), np.float64)
        rc = self._L.lba_optimize_stopflag(C.byref(P), 1, int(iterations), ptr(self._lm_ws), ptr(stats), ptr(stop_flag), stream(win["poses"]))
        if rc != _lib.ORB_E_ABORTED:   # (a raised stop flag ends the optimisation as g2o's terminate() does: the function goes on)
            check(rc, "lba_optimize")
        return stats[0]

    def ComputeErrors(self, win):
        """e->chi2() and the depth of every edge into win["chi2"] / win["depth"] (lba_compute_errors)"""
        P = self._problem(win)
        S = LbaSystem(None, None, None, None, None, None, ptr(win["chi2"]).value, None, ptr(win["depth"]).value, None)
        check(self._L.lba_compute_errors(C.byref(P), 1, C.byref(S), stream(win["poses"])), "lba_compute_errors")

    def Apply(self, view, kfs, win, cap_obs_out=None, out=None):
        """Optimizer.cc:2293-2510 for the window (orbm_lba_window_apply), asynchronously.  view["mp"], view["kf_mp"], kfs["pose"],
        kfs["center"] (KEYFRAME_CENTER_DTYPE [n_kf]), kfs["ref"] (REFRESH_POINT_DTYPE [n_mp]) and kfs["mp_nobs"] (int32 [n_mp], optional) are
        updated in place; win["chi2"] / win["depth"] are read.
        -> dict(erased int32 [cap_e, 2], went_bad int32 [cap_l], obs_start [n_mp + 1], obs [cap_obs_out, 12], result [LBA_A_WORDS])."""
        V, like = self._view(view), view["obs_start"]
        I = self._in(V, kfs)
        cap_obs_out = V.n_obs if cap_obs_out is None else int(cap_obs_out)
        if out is None:
            i32 = lambda *sh: zeros(like, sh, np.int32)   # noqa: E731
            out = dict(erased=i32(self.caps[2], 2), went_bad=i32(self.caps[1]), obs_start=i32(V.n_mp + 1),
                       obs=zeros(like, (max(cap_obs_out, 1), OBSERVATION_DTYPE.itemsize), np.uint8), result=i32(LBA_A_WORDS))
        win["work"] = self._work(view, kfs, V, I, win.get("work"))
        A = LbaApply(_addr(view["mp"]), _addr(view["kf_mp"]), _addr(kfs.get("mp_nobs")), _addr(kfs["ref"]), _addr(kfs["pose"]),
                     _addr(kfs["center"]), _addr(out["erased"]), _addr(out["went_bad"]), _addr(out["obs_start"]), _addr(out["obs"]),
                     _addr(out["result"]), cap_obs_out, 0)
        O = self._window(win)
        check(self._L.orbm_lba_window_apply(C.byref(V), C.byref(I), C.byref(O), ptr(win["chi2"]), ptr(win["depth"]), C.byref(A),
                                            ptr(win["work"]), stream(like)), "orbm_lba_window_apply")
        return out

    def Run(self, view, kfs, current_kf, init_kf_id, stop_flag=None, win=None, work=None, cap_obs_out=None):
        """Optimizer::LocalBundleAdjustment: Build -> (stop flag) -> optimize(5) -> (stop flag: bDoMore) -> optimize(10) -> computeErrors ->
        Apply.  One read of the build's result words, which the solver's own synchronisation pays for.
        -> dict(num_fixedKF, win, out (None where the map stayed untouched), stats, erased [(key frame, point)], went_bad [point]).
        ORB_E_CAPACITY (a window that does not fit, or a reduced system past the solver's budget) leaves the map untouched and is raised."""
        stopped = (lambda: stop_flag is not None and bool(stop_flag[0]))   # noqa: E731
        win = self.Build(view, kfs, current_kf, init_kf_id, win, work)
        r = self.check_build(win)
        res = dict(num_fixedKF=int(r[LBA_R_NUM_FIXED_KF]), win=win, out=None, stats=[], erased=[], went_bad=[])
        if stopped() or int(r[LBA_R_N_EDGES]) == 0:   # (a window without an edge leaves by the early return: the map stays)
            return res
        res["stats"].append(self.Optimize(win, 5, stop_flag))
        if not stopped():
            res["stats"].append(self.Optimize(win, 10, stop_flag))
        self.ComputeErrors(win)
        out = res["out"] = self.Apply(view, kfs, win, cap_obs_out)
        a = to_host(out["result"])
        if int(a[LBA_A_FLAGS]) & (LBA_BAD_INDEX | LBA_UNSUPPORTED):
            raise OrbHipError(_lib.ORB_E_INVALID, "LocalBA: a bad index or a rig record was met and treated as absent (flags %d)" % int(a[LBA_A_FLAGS]))
        res["early_return"] = bool(int(a[LBA_A_FLAGS]) & LBA_EARLY_RETURN)
        res["erased"] = [tuple(int(v) for v in e) for e in to_host(out["erased"])[:int(a[LBA_A_N_ERASED])]]
        res["went_bad"] = [int(p) for p in to_host(out["went_bad"])[:int(a[LBA_A_N_WENT_BAD])]]
        return res
