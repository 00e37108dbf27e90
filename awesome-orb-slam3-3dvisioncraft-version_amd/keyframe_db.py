"""Host-side mirror of ORB_SLAM3::KeyFrameDatabase (reference include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) above the C ABI
(include/orbhip.h "Place recognition"): a key-frame database whose BowVector rows, records and query state live in device slabs, and the two
queries the reference calls, DetectRelocalizationCandidates (:785-897) and DetectNBestCandidates (:614-782).

Slabs are torch CUDA tensors (product path) or numpy arrays (device=None: only meaningful with the emulated test build, whose "device" is host
memory).  The key-frame records (flags, map, seq, covisibles) are kept on the host and uploaded when they changed; the BowVector rows and the
per-slot query state stay on the device."""
import ctypes as C

import numpy as np

from . import _lib
from ._abi import BOWDB_L1_NORM as L1_NORM
from ._abi import BOWDB_QUERY_DTYPE as QUERY_DTYPE
from ._abi import COVIS, KEYFRAME_DTYPE, KF_PRESENT, MAX_CANDIDATES, STATS_DTYPE, QueryBows, View
from ._lib import OrbHipError, check, check_capacity, ptr, stream, to_host, zeros


class Queries:
    """The device query records of one call (bowdb_query) and, for the place-recognition family, the flat conn list."""

    def __init__(self, db, family, n, cap_conn):
        self.family, self.n, self.cap_conn = family, n, cap_conn
        self.records = db._zeros((n, QUERY_DTYPE.itemsize), np.uint8)
        self.conn = db._zeros((max(cap_conn, 1),), np.int32)
        self.n_conn = 0


class KeyFrameDatabase:
    def __init__(self, n_slots, cap_f, n_maps=16, device=None, lib=None):
        """device: a torch device for the product library, None for numpy slabs (emulated build)."""
        self._L = lib if lib is not None else _lib.load()
        self.n_slots, self.cap_f, self.n_maps, self.device = int(n_slots), int(cap_f), int(n_maps), device
        z, rows = self._zeros, max(self.n_slots, 1)   # at least one row is allocated, so that an empty database still has addresses to pass
        # last_query as int64 bit patterns (torch has no uint64 arithmetic; nothing here computes with them)
        self._slabs = dict(bv_word=z((rows, cap_f), np.int32), bv_value=z((rows, cap_f), np.float64), bv_n=z((rows,), np.int32),
                           reloc_query=z((rows,), np.int64), reloc_score=z((rows,), np.float32), place_query=z((rows,), np.int64),
                           place_score=z((rows,), np.float32))
        for name, slab in self._slabs.items():
            setattr(self, name, slab[:self.n_slots])
        self.kf = np.zeros(n_slots, KEYFRAME_DTYPE)          # host copy of the records
        self.kf["covis"] = -1
        self.map_bad = np.zeros(max(n_maps, 1), np.uint8)    # host copy
        self._d_kf, self._d_map_bad = z((max(n_slots, 1), KEYFRAME_DTYPE.itemsize), np.uint8), z((max(n_maps, 1),), np.uint8)
        self._dirty = True
        self._seq = 0
        self._last_id = {"reloc": 0, "place": 0}
        self._work = {}

    # ---------------------------------------------------------------------------------------------------- storage helpers
    def _zeros(self, shape, dtype):
        return zeros(self.device, shape, dtype)

    def _write(self, dst, src):
        """host numpy -> the leading entries of a slab, in place (the slab's address must not change: captured graphs hold it)"""
        src = np.ascontiguousarray(src)
        flat = src.reshape(-1) if src.dtype == np.int32 else src.view(np.uint8).reshape(-1)   # conn lists are int32 slabs, records are byte slabs
        if self.device is None:
            dst.reshape(-1)[:flat.size] = flat
        else:
            import torch
            dst.view(-1)[:flat.size].copy_(torch.from_numpy(flat.copy()))

    def _sync_records(self):
        if self._dirty:
            self._write(self._d_kf, self.kf)
            self._write(self._d_map_bad, self.map_bad)
            self._dirty = False

    def _idx(self, slots):
        s = np.atleast_1d(np.asarray(slots, np.int64))
        if len(s) and (s.min() < 0 or s.max() >= self.n_slots):
            raise OrbHipError(_lib.ORB_E_INVALID, "slot outside [0, %d)" % self.n_slots)
        if self.device is None:
            return s, s
        import torch
        return s, torch.from_numpy(s).to(self.device)

    # ---------------------------------------------------------------------------------------------------- KeyFrameDatabase::add / erase / clear
    def rows(self, start, count=1):
        """Views of `count` consecutive rows from slot `start` for ORBVocabulary.transform(..., bv_out=...) to write the BowVectors into: that
        call is the data movement of KeyFrameDatabase::add (no copy).  cap of the descriptors must equal cap_f."""
        if start < 0 or count < 0 or start + count > self.n_slots:
            raise OrbHipError(_lib.ORB_E_INVALID, "rows outside the database")
        return dict(bv_word=self.bv_word[start:start + count], bv_value=self.bv_value[start:start + count], bv_n=self.bv_n[start:start + count])

    def add(self, slots, map_ids):
        """KeyFrameDatabase::add (:41-49) for key frames whose rows are already written: present, a new seq each in the order given (the position
        at the back of every inverted-file list), query state zeroed."""
        s, ds = self._idx(slots)
        m = np.broadcast_to(np.asarray(map_ids, np.int32), s.shape)
        for i, slot in enumerate(s):
            self._seq += 1
            self.kf[slot]["flags"] |= KF_PRESENT
            self.kf[slot]["map_id"] = m[i]
            self.kf[slot]["seq"] = self._seq
        for a in (self.reloc_query, self.reloc_score, self.place_query, self.place_score):
            a[ds] = 0
        self._dirty = True

    def erase(self, slots):
        """KeyFrameDatabase::erase (:51-72)"""
        s, _ = self._idx(slots)
        self.kf["flags"][s] &= ~np.uint32(KF_PRESENT)
        self._dirty = True

    def clear(self):
        """KeyFrameDatabase::clear (:74-78)"""
        self.kf["flags"] &= ~np.uint32(KF_PRESENT)
        self._dirty = True

    def clear_map(self, map_id):
        """KeyFrameDatabase::clearMap (:80-102)"""
        hit = ((self.kf["flags"] & KF_PRESENT) != 0) & (self.kf["map_id"] == map_id)
        self.kf["flags"][hit] &= ~np.uint32(KF_PRESENT)
        self._dirty = True

    def set_covisibles(self, slots, lists):
        """lists[i] = slots of GetBestCovisibilityKeyFrames(10) of key frame slots[i], in order (at most 10)"""
        s, _ = self._idx(slots)
        for slot, l in zip(s, lists):
            l = list(l)
            if len(l) > COVIS:
                raise OrbHipError(_lib.ORB_E_INVALID, "more than %d covisibles" % COVIS)
            self.kf[slot]["covis"] = -1
            self.kf[slot]["covis"][:len(l)] = l
        self._dirty = True

    def set_map(self, slots, map_ids):
        """KeyFrame::UpdateMap"""
        s, _ = self._idx(slots)
        self.kf["map_id"][s] = np.broadcast_to(np.asarray(map_ids, np.int32), s.shape)
        self._dirty = True

    def set_map_bad(self, map_id, bad=True):
        """Map::SetBad"""
        if not 0 <= map_id < self.n_maps:
            raise OrbHipError(_lib.ORB_E_INVALID, "map outside [0, %d)" % self.n_maps)
        self.map_bad[map_id] = 1 if bad else 0
        self._dirty = True

    # ---------------------------------------------------------------------------------------------------- queries
    def make_queries(self, family, n, cap_conn=0):
        """Device query records for n queries of family "reloc" or "place" (cap_conn: room of the flat conn list); fill with set_queries."""
        if family not in self._last_id:
            raise OrbHipError(_lib.ORB_E_INVALID, "family is 'reloc' or 'place'")
        return Queries(self, family, int(n), int(cap_conn))

    def set_queries(self, Q, ids, map_ids, rows=None, conn=None):
        """Rewrites the records of Q in place (a captured graph sees the new ones on replay).  ids: F->mnId / pKF->mnId, each non-zero and
        greater than every id used before in the family; rows: row of each query's BowVector in the query slab (default 0, 1, ...); conn
        (place family): per query the slots of GetConnectedKeyFrames()."""
        ids = [int(i) for i in ids]
        if len(ids) != Q.n:
            raise OrbHipError(_lib.ORB_E_INVALID, "%d ids for %d queries" % (len(ids), Q.n))
        last = self._last_id[Q.family]
        for i in ids:
            if i <= last or i >= 1 << 64:
                raise OrbHipError(_lib.ORB_E_INVALID, "query id %d: ids are non-zero and increasing within a family (last used: %d)" % (i, last))
            last = i
        rec = np.zeros(Q.n, QUERY_DTYPE)
        rec["id"] = np.array(ids, np.uint64)
        rec["map_id"] = np.broadcast_to(np.asarray(map_ids, np.int32), (Q.n,))
        rec["row"] = np.arange(Q.n) if rows is None else np.asarray(rows, np.int32)
        flat = []
        if conn is not None:
            if Q.family != "place" or len(conn) != Q.n:
                raise OrbHipError(_lib.ORB_E_INVALID, "conn: one list per query of the place family")
            for k, l in enumerate(conn):
                rec["conn_start"][k], rec["conn_n"][k] = len(flat), len(l)
                flat.extend(int(x) for x in l)
            if len(flat) > Q.cap_conn:
                raise OrbHipError(_lib.ORB_E_CAPACITY, "conn lists hold %d slots, cap_conn = %d" % (len(flat), Q.cap_conn))
        self._write(Q.records, rec)
        if flat:
            self._write(Q.conn, np.array(flat, np.int32))
        Q.n_conn = len(flat)
        self._last_id[Q.family] = last
        return Q

    def _view(self):
        self._sync_records()
        p = lambda a: ptr(a).value   # noqa: E731
        S = self._slabs
        return View(p(S["bv_word"]), p(S["bv_value"]), p(S["bv_n"]), p(self._d_kf), p(S["reloc_query"]), p(S["reloc_score"]), p(S["place_query"]),
                    p(S["place_score"]), p(self._d_map_bad), self.n_slots, self.cap_f, self.n_maps, L1_NORM)

    def _workspace(self, nq):
        w = self._work.get(nq)
        if w is None:
            w = self._work[nq] = self._zeros((int(self._L.bowdb_workspace_bytes(self.n_slots, nq)) + 15) // 16 * 2, np.int64)
        return w

    @staticmethod
    def _bows(q_bows):
        w, v, n = q_bows["bv_word"], q_bows["bv_value"], q_bows["bv_n"]
        return QueryBows(ptr(w).value, ptr(v).value, ptr(n).value, int(w.shape[0]), int(w.shape[1]))

    def DetectRelocalizationCandidates(self, Q, q_bows, cap_cand=64, out=None):
        """Q: make_queries("reloc", ...) + set_queries; q_bows: dict with bv_word [R, cap_q], bv_value, bv_n (ORBVocabulary.transform output, or
        rows() of this database).  No host reads, graph-capturable once the workspace and `out` exist (pass the `out` of an earlier call).
        -> dict(cand [n, cap_cand] slots in the reference's order, n_cand, n_required, stats [n, 16] bytes of STATS_DTYPE, cap_cand)."""
        if Q.family != "reloc":
            raise OrbHipError(_lib.ORB_E_INVALID, "queries of the reloc family expected")
        o = out if out is not None else dict(cand=self._zeros((Q.n, max(cap_cand, 1)), np.int32), n_cand=self._zeros((Q.n,), np.int32),
                                             n_required=self._zeros((Q.n,), np.int32), stats=self._zeros((Q.n, 16), np.uint8), cap_cand=cap_cand)
        view, bows = self._view(), self._bows(q_bows)
        check(self._L.bowdb_detect_relocalization_candidates(C.byref(view), ptr(Q.records), Q.n, C.byref(bows), ptr(o["cand"]), o["cap_cand"],
                                                           ptr(o["n_cand"]), ptr(o["n_required"]), ptr(o["stats"]), ptr(self._workspace(Q.n)),
                                                           stream(self.device)), "bowdb_detect_relocalization_candidates failed")
        return o

    def DetectNBestCandidates(self, Q, q_bows, n_candidates=3, out=None):
        """Q: make_queries("place", ...) + set_queries.  -> dict(loop [n, n_candidates] slots (-1 padded), n_loop, merge, n_merge, stats)."""
        if Q.family != "place":
            raise OrbHipError(_lib.ORB_E_INVALID, "queries of the place family expected")
        if not 1 <= n_candidates <= MAX_CANDIDATES:
            raise OrbHipError(_lib.ORB_E_INVALID, "n_candidates outside 1..%d" % MAX_CANDIDATES)
        o = out if out is not None else dict(loop=self._zeros((Q.n, n_candidates), np.int32), n_loop=self._zeros((Q.n,), np.int32),
                                             merge=self._zeros((Q.n, n_candidates), np.int32), n_merge=self._zeros((Q.n,), np.int32),
                                             stats=self._zeros((Q.n, 16), np.uint8), n_candidates=n_candidates)
        view, bows = self._view(), self._bows(q_bows)
        check(self._L.bowdb_detect_n_best_candidates(C.byref(view), ptr(Q.records), Q.n, C.byref(bows), ptr(Q.conn), Q.n_conn, o["n_candidates"],
                                                   ptr(o["loop"]), ptr(o["n_loop"]), ptr(o["merge"]), ptr(o["n_merge"]), ptr(o["stats"]),
                                                   ptr(self._workspace(Q.n)), stream(self.device)), "bowdb_detect_n_best_candidates failed")
        return o

    def check_overflow(self, reloc):
        """Host check (reads n_required back): raises OrbHipError(ORB_E_CAPACITY) if a relocalisation query had more candidates than cap_cand."""
        req = to_host(reloc["n_required"])
        bad = np.nonzero(req > reloc["cap_cand"])[0]
        check_capacity(bad, lambda b: "relocalisation: %d query(ies) have more than cap_cand = %d candidates (query %d: %d)"
                       % (len(bad), reloc["cap_cand"], b, int(req[b])))


def stats_of(result):
    """the stats bytes of a query result as a STATS_DTYPE array"""
    return to_host(result["stats"]).view(STATS_DTYPE).reshape(-1)
