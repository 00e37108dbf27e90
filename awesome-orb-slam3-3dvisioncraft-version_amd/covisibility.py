"""The covisibility graph of the device map (include/orbhip.h "Covisibility graph"): KeyFrame::UpdateConnections, the connection part of
KeyFrame::SetBadFlag and the getters of reference src/KeyFrame.cc:228-330, 427-550, 793-807, above the C ABI.

The store (weight maps as insertion-ordered rows, the two ordered vectors) lives in caller-visible slabs next to the map the other kernels
read; arrays may be torch CUDA tensors (product path) or numpy arrays (the emulated test build).  The getters read rows back to the host."""
import ctypes as C

import numpy as np

from . import _lib
from ._abi import (COVIS_BAD_INDEX, COVIS_CHILD_EVENT_DTYPE, COVIS_ENTRY_DTYPE, COVIS_KEYFRAME_DTYPE, COVIS_KF_FIRST_CONNECTION,  # noqa: F401
                   COVIS_OVERFLOW, CULL_EVENT_DTYPE, CovisOut, CovisStore, CullWorkspaceLayout, LocalMapView)
from ._lib import OrbHipError, check, ptr, stream, to_host, zeros
from .matcher import _addr, _nrec


def flatten_covisibility(keyframes, cap_conn):
    """keyframes: the list flatten_local_map_keyframes takes, every dict with the members of the graph as well: id (mnId, default: the slot),
    map_id (default 0), first_connection (mbFirstConnection, default True), conn = mConnectedKeyFrameWeights as [(kf, weight), ...] in insertion
    order, ordered_kf / ordered_w = mvpOrderedConnectedKeyFrames / mvOrderedWeights.  A row longer than cap_conn is refused.
    -> (ckf COVIS_KEYFRAME_DTYPE [n], dict(conn COVIS_ENTRY_DTYPE [n, cap_conn], n_conn, ordered_kf, ordered_w [n, cap_conn], n_ordered))."""
    n = len(keyframes)
    ckf = np.zeros(n, COVIS_KEYFRAME_DTYPE)
    st = dict(conn=np.zeros((n, cap_conn), COVIS_ENTRY_DTYPE), n_conn=np.zeros(n, np.int32), ordered_kf=np.zeros((n, cap_conn), np.int32),
              ordered_w=np.zeros((n, cap_conn), np.int32), n_ordered=np.zeros(n, np.int32))
    for i, k in enumerate(keyframes):
        if k is None:
            continue
        ckf[i]["id"], ckf[i]["map_id"] = k.get("id", i), k.get("map_id", 0)
        ckf[i]["flags"] = COVIS_KF_FIRST_CONNECTION if k.get("first_connection", True) else 0
        conn, okf, ow = list(k.get("conn", ())), list(k.get("ordered_kf", ())), list(k.get("ordered_w", ()))
        if len(conn) > cap_conn or len(okf) > cap_conn or len(okf) != len(ow):
            raise OrbHipError(_lib.ORB_E_CAPACITY, "covisibility: key frame %d has %d connections, cap_conn = %d" % (i, len(conn), cap_conn))
        for j, (b, w) in enumerate(conn):
            st["conn"][i, j] = (b, w)
        st["n_conn"][i], st["n_ordered"][i] = len(conn), len(okf)
        st["ordered_kf"][i, :len(okf)], st["ordered_w"][i, :len(ow)] = okf, ow
    return ckf, st


class CovisibilityGraph:
    """store: dict(conn [n_kf, cap_conn] of COVIS_ENTRY_DTYPE (torch: uint8 [n_kf, cap_conn, 8]), n_conn int32 [n_kf], ordered_kf / ordered_w
    int32 [n_kf, cap_conn], n_ordered int32 [n_kf]); ckf: COVIS_KEYFRAME_DTYPE [n_kf] (torch: uint8 [n_kf, 16]).  All are updated in place."""

    def __init__(self, store, ckf, *, lib=None):
        self._L = lib if lib is not None else _lib.load()
        self.store, self.ckf = store, ckf
        self.n_kf, self.cap_conn = int(store["ordered_kf"].shape[0]), int(store["ordered_kf"].shape[1])
        if _nrec(ckf) != self.n_kf or _nrec(store["conn"]) != self.n_kf * self.cap_conn or store["ordered_w"].shape != store["ordered_kf"].shape \
                or store["n_conn"].shape[0] != self.n_kf or store["n_ordered"].shape[0] != self.n_kf:
            raise OrbHipError(_lib.ORB_E_INVALID, "covisibility: the slabs of the store and ckf share n_kf and cap_conn")

    def _store(self):
        s = self.store
        return CovisStore(_addr(s["conn"]), _addr(s["n_conn"]), _addr(s["ordered_kf"]), _addr(s["ordered_w"]), _addr(s["n_ordered"]),
                          self.cap_conn, 0)

    def _view(self, view):
        """orbm_localmap_view of the members the graph reads: mp, obs_start, obs, kf, kf_mp, kf_by_order of the dict UpdateLocalMap takes"""
        n_mp = _nrec(view["mp"])
        if _nrec(view["kf"]) != self.n_kf or view["kf_by_order"].shape[0] != self.n_kf or view["obs_start"].shape[0] != n_mp + 1:
            raise OrbHipError(_lib.ORB_E_INVALID, "covisibility: kf and kf_by_order need the store's n_kf entries, obs_start n_mp + 1")
        return LocalMapView(_addr(view["mp"]), _addr(view["obs_start"]), _addr(view["obs"]), _addr(view["kf"]), _addr(view["kf_mp"]), None,
                            _addr(view["kf_by_order"]), None, n_mp, _nrec(view["obs"]), self.n_kf, int(view["kf_mp"].shape[0]), 0, 0)

    def Workspace(self, n_list):
        """uint8 workspace of UpdateConnections for a list of n_list (EraseConnections needs no more), allocated like the store"""
        return zeros(self.store["n_conn"], (max(int(self._L.orbm_covis_workspace_bytes(self.n_kf, int(n_list))), 16),), np.uint8)

    def _work(self, out, work, n_list):
        out["work"] = work if work is not None else out.get("work")
        if out["work"] is None:
            out["work"] = self.Workspace(n_list)
        if out["work"].shape[0] < self._L.orbm_covis_workspace_bytes(self.n_kf, int(n_list)):
            raise OrbHipError(_lib.ORB_E_INVALID, "covisibility: the workspace is too small for this list")

    def UpdateConnections(self, view, kf_list, init_kf_id, work=None, out=None):
        """KeyFrame::UpdateConnections for the key frames of kf_list (int32 [n_list], on the device) IN LIST ORDER (orbm_update_connections),
        asynchronously on the inputs' stream: the store, ckf (the first-connection flag) and view["kf"] (covis, parent) are updated in place.
        -> dict(child_events [n_list, 8] u8 view of COVIS_CHILD_EVENT_DTYPE, n_child_events [1], nmax / kfmax / n_counter [n_list] (n_counter 0 =
        the early return), overflow_kf [1], flags [1] of COVIS_* bits, work).  check_flags() reads the flags back."""
        n_list, like = int(kf_list.shape[0]), self.store["n_conn"]
        if out is None:
            i32 = lambda *sh: zeros(like, sh, np.int32)   # noqa: E731
            out = dict(child_events=zeros(like, (max(n_list, 1), COVIS_CHILD_EVENT_DTYPE.itemsize), np.uint8), n_child_events=i32(1),
                       nmax=i32(max(n_list, 1)), kfmax=i32(max(n_list, 1)), n_counter=i32(max(n_list, 1)), overflow_kf=i32(1), flags=i32(1))
        self._work(out, work, n_list)
        V, S = self._view(view), self._store()
        O = CovisOut(*[_addr(out[k]) for k in ("child_events", "n_child_events", "nmax", "kfmax", "n_counter", "overflow_kf", "flags")])
        check(self._L.orbm_update_connections(C.byref(V), C.byref(S), ptr(self.ckf), ptr(view["kf"]), ptr(kf_list), n_list,
                                              int(init_kf_id) & 0xFFFFFFFF, C.byref(O), ptr(out["work"]), stream(like)), "orbm_update_connections")
        return out

    def EraseConnections(self, view, events=None, n_events=None, kf_erased=None, culled=None, problem=0, work=None, out=None):
        """The connection part of KeyFrame::SetBadFlag for cull events in order (orbm_erase_connections).  Either events (CULL_EVENT_DTYPE
        [cap_events]; torch: uint8 [cap_events, 12]), n_events int32 [1] and optionally kf_erased uint8 [n_kf] (0 = the event was deferred), or
        culled = the dict of ORBmatcher.CullKeyFrames with the problem to fold: its events, count and the workspace's erased bytes are used
        where they lie.  -> dict(flags [1], work)."""
        like = self.store["n_conn"]
        if culled is not None:
            events, n_events = culled["events"][problem], culled["n_events"][problem:problem + 1]
            Y = CullWorkspaceLayout()
            check(self._L.orbm_cull_workspace(self.n_kf, _nrec(view["mp"]), _nrec(view["obs"]), C.byref(Y)), "orbm_cull_workspace")
            off = problem * Y.stride + Y.kf_erased
            kf_erased = culled["work"][off:off + max(self.n_kf, 1)]
        if out is None:
            out = dict(flags=zeros(like, (1,), np.int32))
        self._work(out, work, 0)
        V, S = self._view(view), self._store()
        O = CovisOut(None, None, None, None, None, None, _addr(out["flags"]))
        check(self._L.orbm_erase_connections(C.byref(V), C.byref(S), ptr(view["kf"]), ptr(events), ptr(n_events), ptr(kf_erased), _nrec(events),
                                             C.byref(O), ptr(out["work"]), stream(like)), "orbm_erase_connections")
        return out

    def check_flags(self, out):
        """Host check (reads the flag word back): OrbHipError(ORB_E_INVALID) for a bad index, OrbHipError(ORB_E_CAPACITY) for a dropped insert."""
        fl = int(to_host(out["flags"])[0])
        if fl & COVIS_BAD_INDEX:
            raise OrbHipError(_lib.ORB_E_INVALID, "covisibility: a bad index was met and treated as absent")
        if fl & COVIS_OVERFLOW:
            raise OrbHipError(_lib.ORB_E_CAPACITY, "covisibility: the row of key frame %d does not fit cap_conn = %d"
                              % (int(to_host(out["overflow_kf"])[0]) if "overflow_kf" in out else -1, self.cap_conn))

    # -- the getters (KeyFrame.cc:275-330): they read the key frame's rows back
    def _ordered(self, kf):
        n = int(to_host(self.store["n_ordered"][kf:kf + 1])[0])
        return to_host(self.store["ordered_kf"][kf, :n]).tolist(), to_host(self.store["ordered_w"][kf, :n]).tolist()

    def GetVectorCovisibleKeyFrames(self, kf):
        return self._ordered(kf)[0]

    def GetBestCovisibilityKeyFrames(self, kf, N):
        return self._ordered(kf)[0][:max(int(N), 0)]

    def GetCovisiblesByWeight(self, kf, w):
        okf, ow = self._ordered(kf)
        if not okf:
            return []
        it = next((i for i, x in enumerate(ow) if w > x), len(ow))   # upper_bound(.., w, weightComp), weightComp(a, b) = a > b
        if it == len(ow) and ow[-1] < w:
            return []
        return okf[:it]

    def GetWeight(self, kf, other):
        n = int(to_host(self.store["n_conn"][kf:kf + 1])[0])
        row = to_host(self.store["conn"][kf, :n])
        if not isinstance(row, np.ndarray) or not row.dtype.names:
            row = np.ascontiguousarray(row).view(COVIS_ENTRY_DTYPE).reshape(-1)
        hit = np.nonzero(row["kf"] == other)[0]
        return int(row["weight"][hit[0]]) if len(hit) else 0
