"""The covisibility graph on the device map (include/orbhip.h "Covisibility graph"): orbm_update_connections and orbm_erase_connections against a
literal Python restatement of KeyFrame::UpdateConnections (KeyFrame.cc:427-550), AddConnection (:228-241), UpdateBestCovisibles (:243-265) and the
connection part of SetBadFlag (:675-678, 696-697) with EraseConnection (:793-807), written over dicts and lists as the reference holds them;
pointer order is a random permutation.  Integer work: every slab is compared whole, bit for bit, the bytes past the counts against a sentinel.
Every constructed case is also run through deliberately wrong variants OF THE RESTATEMENT, so that the case is known to discriminate."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import orbhip
from devarrays import BACKENDS, lib, to_dev, to_dev_plain, to_host  # noqa: F401
from orbhip._abi import (COVIS_BAD_INDEX, COVIS_ENTRY_DTYPE, COVIS_KF_FIRST_CONNECTION, COVIS_OVERFLOW, CULL_EVENT_DTYPE, CULL_MONOCULAR,
                         CULL_PROBLEM_DTYPE, LM_KF_BAD, LOCALMAP_FRAME_DTYPE, LOCALMAP_KEYFRAME_DTYPE, MAP_POINT_DTYPE, MP_BAD, MP_VALID, OBS_RIGHT,
                         ORB_E_INVALID, REFRESH_POINT_DTYPE, TRACK_DTYPE, CovisOut, CovisStore, LocalMapView)
from orbhip.covisibility import CovisibilityGraph, flatten_covisibility
from orbhip.matcher import flatten_cull_keyframes, flatten_local_map_keyframes, flatten_observations

SENT8 = 0x5A
SENT32 = 0x5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH = 15
INIT_NONE = 0xFFFFFFF0   # an init id no key frame has


# ------------------------------------------------------------------------------------------------ a map as the reference holds it
class World:
    """kfs: per slot None or dict(id, map_id, bad, mp = mvpMapPoints as point indices (None = NULL), first = mbFirstConnection, parent, conn =
    mConnectedKeyFrameWeights as an insertion-ordered dict, okf / ow = the two ordered vectors).  mps: dict(bad, obs = the key frames of
    mObservations in its iteration order, which is pointer order, right = those whose entry has a rightIndex too).  order = d_kf_by_order."""

    def __init__(self, kf_points, n_mp, order=None, rng=None, bad_kf=(), bad_mp=(), ids=None, map_ids=None, no_obs=(), extra_obs=(), right=(),
                 empty=(), cap_conn=None):
        n = len(kf_points)
        self.order = list(order) if order is not None else (list(rng.permutation(n)) if rng is not None else list(range(n)))
        self.rank = {int(k): r for r, k in enumerate(self.order)}
        self.kfs = [None if k in empty else dict(id=ids[k] if ids else k, map_id=map_ids[k] if map_ids else 0, bad=k in bad_kf, mp=list(kf_points[k]),
                                                 first=True, parent=None, conn={}, okf=[], ow=[]) for k in range(n)]
        self.mps = [dict(bad=p in bad_mp, obs=[], right=set()) for p in range(n_mp)]
        for k in sorted(range(n), key=lambda k: self.rank[k]):
            if self.kfs[k] is None:
                continue
            for p in self.kfs[k]["mp"]:
                if p is not None and 0 <= p < n_mp and (k, p) not in no_obs and k not in self.mps[p]["obs"]:
                    self.mps[p]["obs"].append(k)
        for p, k in extra_obs:
            self.mps[p]["obs"].append(k)
            self.mps[p]["obs"].sort(key=lambda k: self.rank[k])
        for p, k in right:
            self.mps[p]["right"].add(k)
        self.cap_conn = cap_conn or max(n - 1, 1) + 2
        self.raw = None        # the rows of the store as the device holds them, stale entries included: set by flatten()
        self.rebuilt = set()   # key frames whose ordered vectors were written
        self.stats = dict(unchanged=0, sub_listed=0, stamp_kept=0, none15=0)

    # the row of d_conn as an insertion-ordered map: what the restatement's dict operations do to the stored bytes
    def row_assign(self, k):
        for j, e in enumerate(self.kfs[k]["conn"].items()):
            if self.raw is not None and j < self.cap_conn:
                self.raw[k][j] = e

    def row_erase(self, k, key):
        conn = self.kfs[k]["conn"]
        at, n = list(conn).index(key), len(conn)
        del conn[key]
        if self.raw is not None and n <= self.cap_conn:
            self.raw[k][at:n - 1] = self.raw[k][at + 1:n]


def update_best_covisibles(W, b, variant=None, is_bad=None, trigger=None):
    """KeyFrame::UpdateBestCovisibles of key frame b"""
    B = W.kfs[b]
    is_bad = is_bad or (lambda k: W.kfs[k]["bad"])
    vPairs = sorted(((w, k) for k, w in B["conn"].items()), key=lambda t: (t[0], -W.rank[t[1]] if variant == "asc_ties" else W.rank[t[1]]))
    lKFs, lWs = [], []
    for w, k in vPairs:
        if not is_bad(k):
            lKFs.insert(0, k)
            lWs.insert(0, w)
            if w < TH and k != trigger:
                W.stats["sub_listed"] += 1
    B["okf"], B["ow"] = lKFs, lWs
    W.rebuilt.add(b)


def add_connection(W, b, a, weight, variant=None):
    """KeyFrame::AddConnection: b->AddConnection(a, weight)"""
    B = W.kfs[b]
    if a not in B["conn"]:
        B["conn"][a] = weight
    elif B["conn"][a] != weight:
        B["conn"][a] = weight
    else:
        W.stats["unchanged"] += 1
        if variant != "always_rebuild":
            return
    W.row_assign(b)   # (a new key lands at the end, an overwritten one keeps its place: the other entries are rewritten as they are)
    update_best_covisibles(W, b, variant, trigger=a)


def update_connections(W, a, init_id, variant=None):
    """KeyFrame::UpdateConnections of key frame a -> dict(n_counter, nmax, kfmax, event)"""
    A = W.kfs[a]
    KFcounter = {}
    points = A["mp"] if variant != "count_once" else list(dict.fromkeys(A["mp"]))
    for p in points:
        if p is None:
            continue
        m = W.mps[p]
        if m["bad"]:
            continue
        for k in m["obs"]:
            K = W.kfs[k]
            if K["id"] == A["id"] or K["bad"] or K["map_id"] != A["map_id"]:
                continue
            KFcounter[k] = KFcounter.get(k, 0) + 1
    if not KFcounter:
        return dict(n_counter=0, nmax=0, kfmax=-1, event=None)
    KFcounter = {k: KFcounter[k] for k in sorted(KFcounter, key=lambda k: W.rank[k])}   # a std::map<KeyFrame*, int>
    nmax, pKFmax, vPairs = 0, None, []
    for k, c in KFcounter.items():
        if c > nmax:
            nmax, pKFmax = c, k
        if (c > TH) if variant == "gt" else (c >= TH):
            vPairs.append((c, k))
            add_connection(W, k, a, c, variant)
    if not vPairs:
        W.stats["none15"] += 1
        vPairs.append((nmax, pKFmax))
        add_connection(W, pKFmax, a, nmax, variant)
    vPairs.sort(key=lambda t: (t[0], -W.rank[t[1]] if variant == "asc_ties" else W.rank[t[1]]))
    lKFs, lWs = [], []
    for w, k in vPairs:
        lKFs.insert(0, k)
        lWs.insert(0, w)
    A["conn"] = dict(KFcounter) if variant != "own_filtered" else {k: c for k, c in KFcounter.items() if c >= TH}
    W.row_assign(a)
    A["okf"], A["ow"] = lKFs, lWs
    W.rebuilt.add(a)
    event = None
    if A["first"] and A["id"] != init_id:
        A["parent"] = lKFs[0]
        A["first"] = False
        event = (a, lKFs[0])
    return dict(n_counter=len(KFcounter), nmax=nmax, kfmax=pKFmax, event=event)


def erase_connections(W, events, variant=None):
    """the connection part of KeyFrame::SetBadFlag for each (kf, erased) event in order; erased False = mbNotErase deferred it"""
    final_bad = {k for k, erased in events if erased}
    later = set(final_bad)
    for k, erased in events:
        if not erased:
            continue
        K = W.kfs[k]
        later.discard(k)

        def is_bad(x):
            if variant == "final_bad":
                return W.kfs[x]["bad"] or x in final_bad
            if x in later and x != k:
                W.stats["stamp_kept"] += 1
            return W.kfs[x]["bad"]
        for b in list(K["conn"]):
            B = W.kfs[b]
            if k in B["conn"]:   # EraseConnection
                W.row_erase(b, k)
                update_best_covisibles(W, b, is_bad=is_bad)
        K["conn"] = {}
        K["okf"], K["ow"] = [], []   # (the reference leaves mvOrderedWeights behind; no getter reads it past the empty vector)
        W.rebuilt.add(k)
        K["bad"] = True


def state(W):
    return [None if k is None else (list(k["conn"].items()), k["okf"], k["ow"], k["parent"], k["first"]) for k in W.kfs]


# ------------------------------------------------------------------------------------------------ flattening and running
def flatten(W, stale_covis=False):
    """the device arrays of W, the store's unused entries filled with the sentinel"""
    recs = [None if k is None else dict(bad=k["bad"], parent=-1 if k["parent"] is None else k["parent"], mp=[-1 if p is None else p for p in k["mp"]],
                                        covis=k["okf"][:10], id=k["id"], map_id=k["map_id"], first_connection=k["first"],
                                        conn=list(k["conn"].items()), ordered_kf=k["okf"], ordered_w=k["ow"]) for k in W.kfs]
    kf, kf_mp, _ = flatten_local_map_keyframes(recs)
    ckf, st = flatten_covisibility(recs, W.cap_conn)
    for k in range(len(W.kfs)):
        st["conn"][k, st["n_conn"][k]:] = (SENT32, SENT32)
        st["ordered_kf"][k, st["n_ordered"][k]:] = SENT32
        st["ordered_w"][k, st["n_ordered"][k]:] = SENT32
    W.raw = [[tuple(int(x) for x in e) for e in st["conn"][k]] for k in range(len(W.kfs))]
    row0 = np.concatenate([[0], np.cumsum([0 if k is None else len(k["mp"]) for k in W.kfs])])

    def desc_row(k, p):   # one descriptor row per feature in key-frame order: the first feature that holds the point is the entry's leftIndex
        return int(row0[k]) + (W.kfs[k]["mp"].index(p) if W.kfs[k] is not None and p in W.kfs[k]["mp"] else 0)
    obs_start, obs = flatten_observations([[r for k in m["obs"] for r in [(k, desc_row(k, p), 0)] + ([(k, desc_row(k, p), OBS_RIGHT)] if k in m["right"] else [])]
                                           for p, m in enumerate(W.mps)])
    mp = np.zeros(len(W.mps), MAP_POINT_DTYPE)
    mp["flags"] = [MP_VALID | (MP_BAD if m["bad"] else 0) for m in W.mps]
    view = dict(mp=mp, obs_start=obs_start, obs=obs, kf=kf, kf_mp=kf_mp, kf_by_order=np.asarray(W.order, np.int32).reshape(-1))
    return view, ckf, st


def rec_dev(a, backend):
    if backend == "hip" and a.size == 0:
        import torch
        return torch.zeros(a.shape + (a.dtype.itemsize,), dtype=torch.uint8, device="cuda")
    return to_dev(a.copy(), backend)


def upload(view, ckf, st, backend):
    dv = {k: (rec_dev(v, backend) if v.dtype.names else to_dev_plain(v.copy(), backend)) for k, v in view.items()}
    ds = {k: (rec_dev(v, backend) if v.dtype.names else to_dev_plain(v.copy(), backend)) for k, v in st.items()}
    return dv, rec_dev(ckf, backend), ds


def sync(backend):
    if backend == "hip":
        import torch
        torch.cuda.synchronize()


def u8(a):
    a = to_host(a)
    return a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,)) if a.dtype.names else a


def sentinel_out(n_list, backend):
    n = max(n_list, 1)
    i32 = lambda *sh: to_dev_plain(np.full(sh, SENT32, np.int32), backend)   # noqa: E731
    return dict(child_events=to_dev_plain(np.full((n, 8), SENT8, np.uint8), backend), n_child_events=i32(1), nmax=i32(n), kfmax=i32(n),
                n_counter=i32(n), overflow_kf=i32(1), flags=i32(1))


def check_store(W, view0, ckf0, st0, dv, dckf, ds, skip_rows=()):
    """every slab of the device against the restatement's world W (view0 / ckf0 / st0: the arrays before the call)"""
    n_kf, cap = len(W.kfs), W.cap_conn
    want = {k: v.copy() for k, v in st0.items()}
    kf, ckf = view0["kf"].copy(), ckf0.copy()
    for k, K in enumerate(W.kfs):
        if K is None:
            continue
        ckf[k]["flags"] = COVIS_KF_FIRST_CONNECTION if K["first"] else 0
        if k in skip_rows:
            continue
        want["conn"][k] = np.asarray(W.raw[k], np.int64).astype(np.int32).view(COVIS_ENTRY_DTYPE).reshape(-1) if cap else want["conn"][k]
        want["n_conn"][k] = len(K["conn"])
        if k in W.rebuilt:   # only the last rebuild is written: nothing behind its count
            n = len(K["okf"])
            want["ordered_kf"][k, :n], want["ordered_w"][k, :n], want["n_ordered"][k] = K["okf"], K["ow"], n
            kf[k]["covis"] = (K["okf"][:10] + [-1] * 10)[:10]
        else:
            assert list(st0["ordered_kf"][k, :st0["n_ordered"][k]]) == K["okf"]
        kf[k]["parent"] = -1 if K["parent"] is None else K["parent"]
        ckf[k]["flags"] = COVIS_KF_FIRST_CONNECTION if K["first"] else 0
    got = {k: to_host(v) for k, v in ds.items()}
    got["conn"] = u8(ds["conn"]).reshape(n_kf, cap, 8)
    want["conn"] = u8(want["conn"]).reshape(n_kf, cap, 8)
    keep = [k for k in range(n_kf) if k not in skip_rows]
    for name in ("n_conn", "conn", "n_ordered", "ordered_kf", "ordered_w"):
        assert np.array_equal(got[name][keep], want[name][keep]), (name, [k for k in keep if not np.array_equal(got[name][k], want[name][k])][:5])
    got_kf = u8(dv["kf"]).reshape(n_kf, -1)
    assert np.array_equal(got_kf[keep], u8(kf).reshape(n_kf, -1)[keep]), "kf"
    assert np.array_equal(u8(dckf).reshape(n_kf, -1), u8(ckf).reshape(n_kf, -1)), "ckf"
    for name in ("mp", "obs_start", "obs", "kf_mp", "kf_by_order"):   # inputs untouched
        assert np.array_equal(u8(dv[name]), u8(view0[name])), name


def run_update(lib, backend, W0, kf_list, init_id=INIT_NONE, corrupt=None, absent=None, expect_flags=0, variants=(), skip_rows=(),
               overflow_kf=-1, twice=False):
    """Runs orbm_update_connections on the flattened W0 and compares every slab and output with the restatement run on a copy of W0 (of
    absent(copy) where `corrupt` damages the flattened arrays).  variants: wrong variants of the restatement that must give another outcome.
    -> (the restatement's world, its per-entry results, the graph object, the device view)"""
    view, ckf, st = flatten(W0)
    lst = np.asarray(list(kf_list), np.int32).reshape(-1)
    if corrupt:
        corrupt(view, ckf, st, lst)
    dv, dckf, ds = upload(view, ckf, st, backend)
    G = CovisibilityGraph(ds, dckf, lib=lib)
    out = G.UpdateConnections(dv, to_dev_plain(lst, backend), init_id, out=sentinel_out(len(lst), backend))
    sync(backend)
    W = copy.deepcopy(W0)
    if absent:
        W = absent(W) or W
    res = [update_connections(W, int(a), init_id) if 0 <= a < len(W.kfs) and W.kfs[a] is not None else dict(n_counter=0, nmax=0, kfmax=-1, event=None)
           for a in kf_list]
    n = len(lst)
    if n:
        for name in ("nmax", "kfmax", "n_counter"):
            assert list(to_host(out[name])[:n]) == [r[name] for r in res], (name, list(to_host(out[name])[:n]), [r[name] for r in res])
            assert np.all(to_host(out[name])[n:] == SENT32)
        events = [r["event"] for r in res if r["event"]]
        want = np.full((max(n, 1), 8), SENT8, np.uint8)
        if events:
            want[:len(events)] = np.asarray(events, np.int32).view(np.uint8).reshape(-1, 8)
        assert int(to_host(out["n_child_events"])[0]) == len(events) and np.array_equal(to_host(out["child_events"]), want), events
        assert int(to_host(out["flags"])[0]) == expect_flags, int(to_host(out["flags"])[0])
        assert int(to_host(out["overflow_kf"])[0]) == overflow_kf
        if expect_flags:
            with pytest.raises(orbhip.OrbHipError):
                G.check_flags(out)
        else:
            G.check_flags(out)
    else:
        for name in out:   # a no-op: nothing is written
            if name != "work":
                assert np.all(to_host(out[name]).view(np.uint8) == SENT8), name
    check_store(W, view, ckf, st, dv, dckf, ds, skip_rows)
    for v in variants:
        X = copy.deepcopy(W0)
        X.raw = None
        rv = [update_connections(X, int(a), init_id, variant=v) for a in kf_list]
        assert state(X) != state(W) or rv != res, v
    return W, res, G, dv


def run_erase(lib, backend, W0, events, pass_erased=True, flag_bad=False, corrupt=None, expect_flags=0, variants=(), cap_events=None):
    """events: [(kf, erased)] in order.  flag_bad: the view already carries ORBM_LM_KF_BAD for the erased key frames (the call after the apply).
    -> (the restatement's world, the device store as host arrays)"""
    view, ckf, st = flatten(W0)
    if flag_bad:
        for k, erased in events:
            if erased:
                view["kf"][k]["flags"] |= LM_KF_BAD
    cap_events = cap_events if cap_events is not None else len(events) + 2
    ev = np.full(cap_events, -1, CULL_EVENT_DTYPE)
    ev["kf"][:len(events)] = [k for k, _ in events][:cap_events]
    n_ev = np.asarray([len(events)], np.int32)
    erased = np.zeros(max(len(W0.kfs), 1), np.uint8)
    for k, e in events:
        erased[k] |= 1 if e else 0
    if corrupt:
        corrupt(view, ckf, st, ev, n_ev)
    dv, dckf, ds = upload(view, ckf, st, backend)
    G = CovisibilityGraph(ds, dckf, lib=lib)
    out = G.EraseConnections(dv, rec_dev(ev, backend), to_dev_plain(n_ev, backend), to_dev_plain(erased, backend) if pass_erased else None,
                             out=dict(flags=to_dev_plain(np.full(1, SENT32, np.int32), backend)))
    sync(backend)
    assert int(to_host(out["flags"])[0]) == expect_flags
    W = copy.deepcopy(W0)
    erase_connections(W, [(k, e or not pass_erased) for k, e in events if 0 <= k < len(W.kfs) and W.kfs[k] is not None][:cap_events])
    check_store(W, view, ckf, st, dv, dckf, ds)   # (the bad flags of d_kf are the apply's to write: the slab is compared as it was)
    for v in variants:
        X = copy.deepcopy(W0)
        X.raw = None
        erase_connections(X, events, variant=v)
        Y = copy.deepcopy(W0)
        Y.raw = None
        erase_connections(Y, events)
        assert state(X) != state(Y), v
    return W, {k: to_host(v).copy() for k, v in ds.items()}


# ------------------------------------------------------------------------------------------------ constructed worlds
def shared(counts, n_extra_feat=0, dup=None, **kw):
    """Key frame 0 (A) shares counts[j] points with key frame j + 1, each point with that one key frame only; dup = {j: d}: A holds the first d
    of those points twice.  -> (kf_points, n_mp)"""
    A, kfs, p = [], [], 0
    for j, c in enumerate(counts):
        pts = list(range(p, p + c))
        p += c
        A += pts + pts[:(dup or {}).get(j, 0)]
        kfs.append(pts)
    A += [None] * n_extra_feat
    return [A] + kfs, p


def preload(W, k, conn, rebuild=True):
    """key frame k starts with this weight map (and the ordered vectors UpdateBestCovisibles gives for it)"""
    W.kfs[k]["conn"] = dict(conn)
    if rebuild:
        update_best_covisibles(W, k)
        W.rebuilt.discard(k)
    W.stats = dict(unchanged=0, sub_listed=0, stamp_kept=0, none15=0)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("nf", [0, 1, 63, 64, 65, 257])
def test_features_per_key_frame(lib, backend, nf):
    """A has nf features, the last of which holds point 0 again; B holds all of A's points (and C half of them): one lane per feature, 256
    per workgroup"""
    rng = np.random.default_rng(nf)
    kfp = [list(range(nf - 1)) + [0] if nf > 1 else list(range(nf)), list(range(nf)), list(range(nf // 2)), []]
    W, res, _, _ = run_update(lib, backend, World(kfp, max(nf, 1), rng=rng), [0], variants=[[], ["own_filtered"]][nf] if nf < 2 else ["count_once"])
    assert res[0]["n_counter"] == (0 if nf == 0 else (1 if nf == 1 else 2)) and res[0]["nmax"] == nf
    if nf == 0:
        assert W.kfs[0]["first"] and not W.rebuilt


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n_kf", [2, 64, 65, 300])
def test_key_frame_counts(lib, backend, n_kf):
    """every key frame shares points with A, 13 + (j % 5) of them: the counter spans more than one chunk of ranks and one wave of targets"""
    rng = np.random.default_rng(n_kf)
    kfp, n_mp = shared([13 + (j % 5) for j in range(n_kf - 1)])
    W, res, _, _ = run_update(lib, backend, World(kfp, n_mp, rng=rng), [0], variants=["gt", "own_filtered", "asc_ties"] if n_kf > 2 else [])
    assert res[0]["n_counter"] == n_kf - 1 and len(W.kfs[0]["conn"]) == n_kf - 1
    assert len(W.kfs[0]["okf"]) == sum(13 + (j % 5) >= 15 for j in range(n_kf - 1)) or n_kf == 2


@pytest.mark.parametrize("backend", BACKENDS)
def test_own_row_over_three_chunks_of_ranks(lib, backend):
    """513 ranks through the 256-lane chunk loop that writes A's own row (csrc/wg_scan.inc): the third chunk writes the per-wave totals where
    the first did.  About a third of the key frames, an irregular set, share nothing with A, so every chunk keeps some entries and drops some;
    the key frame at the last rank, alone in the third chunk, is kept"""
    rng = np.random.default_rng(513)
    n_kf = 513
    order = [int(k) for k in rng.permutation(n_kf)]
    if order[512] == 0:
        order[511], order[512] = order[512], order[511]
    counts = [0 if rng.random() < 0.3 and j + 1 != order[512] else 13 + (j % 5) for j in range(n_kf - 1)]
    kept = sum(c > 0 for c in counts)
    in_chunk = [sum(k != 0 and counts[k - 1] > 0 for k in order[c0:c0 + 256]) for c0 in (0, 256, 512)]
    assert kept % 64 and 0 < in_chunk[0] < 255 and 0 < in_chunk[1] < 255 and in_chunk[2] == 1, (kept, in_chunk)
    kfp, n_mp = shared(counts)
    W, res, _, _ = run_update(lib, backend, World(kfp, n_mp, order=order), [0], variants=["gt", "own_filtered", "asc_ties"])
    assert res[0]["n_counter"] == kept and list(W.kfs[0]["conn"]) == [k for k in order if k != 0 and counts[k - 1] > 0]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n_row", [0, 1, 63, 64, 65])
def test_target_row_lengths(lib, backend, n_row):
    """B's row holds n_row other entries before A is appended, and again with A somewhere inside it (an overwrite that keeps its place)"""
    rng = np.random.default_rng(100 + n_row)
    n_kf = n_row + 3
    kfp = [list(range(14)), list(range(14))] + [[] for _ in range(n_kf - 2)]   # 14: nobody reaches 15, B is connected as the maximum
    for inside in (False, True):
        W0 = World(kfp, 14, rng=rng, cap_conn=n_row + 2)
        others = [(k, 3 + int(rng.integers(0, 40))) for k in range(2, 2 + n_row)]
        if inside and n_row:
            others.insert(n_row // 2, (0, 7))
        preload(W0, 1, others)
        W, _, _, _ = run_update(lib, backend, W0, [0], variants=["own_filtered"])
        assert W.kfs[1]["conn"][0] == 14 and len(W.kfs[1]["okf"]) == n_row + 1 and list(W.kfs[1]["conn"]).index(0) == (n_row // 2 if inside else n_row)


@pytest.mark.parametrize("backend", BACKENDS)
def test_row_capacity_and_overflow(lib, backend):
    """cap_conn entries fit; the insert that would be entry cap_conn + 1 is dropped and flagged, the key frame reported, every other row exact"""
    rng = np.random.default_rng(7)
    kfp = [list(range(20)), list(range(20)), list(range(20)), [], [], []]
    W0 = World(kfp, 20, rng=rng, cap_conn=3)
    preload(W0, 1, [(3, 5), (4, 6)])          # room for one more: fits exactly
    preload(W0, 2, [(3, 5), (4, 6), (5, 9)])  # full: A's entry is dropped
    W, _, G, _ = run_update(lib, backend, W0, [0], expect_flags=COVIS_OVERFLOW, skip_rows={2}, overflow_kf=2)
    assert len(W.kfs[1]["conn"]) == 3
    # the own row: a counter of 4 entries in a row of 3
    kfp, n_mp = shared([16, 17, 18, 19])
    run_update(lib, backend, World(kfp, n_mp, rng=rng, cap_conn=3), [0], expect_flags=COVIS_OVERFLOW, skip_rows={0}, overflow_kf=0)


@pytest.mark.parametrize("backend", BACKENDS)
def test_list_lengths(lib, backend):
    """0 (a no-op: nothing written), 1, the same key frame twice with another between, 70 (the loop of CorrectLoop)"""
    rng = np.random.default_rng(8)
    n_kf = 75
    kfp = [[int(p) for p in rng.choice(400, 60, replace=False)] for _ in range(n_kf)]
    W0 = World(kfp, 400, rng=rng)
    run_update(lib, backend, W0, [])
    run_update(lib, backend, W0, [5], variants=["own_filtered"])
    kfp2, n_mp = shared([10], dup={0: 10})
    W, res, _, _ = run_update(lib, backend, World(kfp2, n_mp, rng=rng), [0, 1, 0], variants=["count_once"])
    assert [r["nmax"] for r in res] == [20, 10, 20] and W.kfs[0]["conn"] == {1: 20} and W.kfs[1]["conn"] == {0: 20}
    W, res, _, _ = run_update(lib, backend, W0, [int(k) for k in rng.permutation(n_kf)[:70]], variants=["own_filtered"])
    assert sum(r["event"] is not None for r in res) == 70


@pytest.mark.parametrize("backend", BACKENDS)
def test_threshold_14_15_and_own_map(lib, backend):
    """counts 14, 15, 16, 3: 15 is connected and 14 is not (>=); the own map keeps all four"""
    kfp, n_mp = shared([14, 15, 16, 3])
    W, res, _, _ = run_update(lib, backend, World(kfp, n_mp, order=[3, 0, 4, 1, 2]), [0], variants=["gt", "own_filtered"])
    A = W.kfs[0]
    assert A["conn"] == {4: 3, 1: 14, 2: 15, 3: 16} and list(A["conn"]) == [3, 4, 1, 2] and A["okf"] == [3, 2] and A["ow"] == [16, 15]
    assert W.kfs[1]["conn"] == {} and W.kfs[2]["conn"] == {0: 15} and W.kfs[4]["conn"] == {}
    assert res[0]["event"] == (0, 3) and A["parent"] == 3 and not A["first"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_nobody_reaches_15(lib, backend):
    """the single maximum is used; a tie at the maximum goes to the first in pointer order"""
    kfp, n_mp = shared([7, 9, 9, 4])
    for order, first in (([0, 1, 2, 3, 4], 2), ([0, 4, 3, 2, 1], 3)):
        W, res, _, _ = run_update(lib, backend, World(kfp, n_mp, order=order), [0], variants=["own_filtered"])
        assert res[0]["nmax"] == 9 and res[0]["kfmax"] == first and W.kfs[0]["okf"] == [first] and W.kfs[0]["ow"] == [9]
        assert W.kfs[first]["conn"] == {0: 9} and W.kfs[5 - first]["conn"] == {} and len(W.kfs[0]["conn"]) == 4 and W.stats["none15"] == 1


@pytest.mark.parametrize("backend", BACKENDS)
def test_empty_counter_leaves_everything(lib, backend):
    """no observer counts: the early return; A's stale map and list, and its first-connection flag, stay"""
    kfp = [[0, 1, None], [5], [6]]
    W0 = World(kfp, 8, no_obs={(1, 5)})
    preload(W0, 0, [(1, 33), (2, 4)])
    W, res, _, _ = run_update(lib, backend, W0, [0, 1])
    assert res[0]["n_counter"] == 0 and W.kfs[0]["conn"] == {1: 33, 2: 4} and W.kfs[0]["okf"] == [1, 2] and W.kfs[0]["first"]
    assert res[0]["event"] is None and not W.rebuilt


@pytest.mark.parametrize("backend", BACKENDS)
def test_sub_threshold_entry_surfaces(lib, backend):
    """B's own map holds a count-3 entry of C that its list lacks.  A's update changes B.map[A]: B is rebuilt from its WHOLE map and now lists
    C.  With the weight unchanged B is not rebuilt and does not"""
    kfp = [list(range(20)), list(range(20)) + [30, 31, 32] + list(range(40, 56)), [30, 31, 32], list(range(40, 56))]
    for old_w, listed in ((19, True), (20, False)):
        W0 = World(kfp, 60, order=[2, 0, 3, 1])
        update_connections(W0, 1, INIT_NONE)   # B's own update: map {A: 20, C: 3, D: 16}, list [A, D]
        assert W0.kfs[1]["conn"] == {2: 3, 0: 20, 3: 16} and W0.kfs[1]["okf"] == [0, 3]
        W0.kfs[1]["conn"][0] = old_w
        W0.kfs[1]["ow"][0] = old_w
        W0.kfs[0]["conn"], W0.kfs[0]["okf"], W0.kfs[0]["ow"] = {}, [], []
        W0.rebuilt, W0.kfs[1]["first"], W0.kfs[1]["parent"] = set(), True, None
        W0.stats["sub_listed"] = W0.stats["unchanged"] = 0
        W, _, _, _ = run_update(lib, backend, W0, [0], variants=["always_rebuild"] if not listed else [])
        assert W.kfs[1]["okf"] == ([0, 3, 2] if listed else [0, 3]) and W.stats["sub_listed"] == (1 if listed else 0)
        assert W.stats["unchanged"] == (0 if listed else 1)


@pytest.mark.parametrize("backend", BACKENDS)
def test_stale_entry_survives(lib, backend):
    """B.map[A] = 20 from an earlier update; A now shares 10 points with B and 16 with C: nothing lowers or removes B.map[A]"""
    kfp, n_mp = shared([10, 16])
    W0 = World(kfp, n_mp)
    preload(W0, 1, [(0, 20)])
    W, _, _, _ = run_update(lib, backend, W0, [0], variants=["own_filtered"])
    assert W.kfs[1]["conn"] == {0: 20} and W.kfs[1]["okf"] == [0] and W.kfs[0]["conn"] == {1: 10, 2: 16} and W.kfs[0]["okf"] == [2]


@pytest.mark.parametrize("backend", BACKENDS)
def test_equal_weights_descending_rank(lib, backend):
    """four connections of weight 17 and one of 18: ties by pointer order DESCENDING; the parent is the front of the list"""
    kfp, n_mp = shared([17, 17, 18, 17, 17])
    W, res, _, _ = run_update(lib, backend, World(kfp, n_mp, order=[4, 2, 0, 5, 1, 3]), [0], variants=["asc_ties"])
    assert W.kfs[0]["okf"] == [3, 1, 5, 2, 4] and W.kfs[0]["ow"] == [18, 17, 17, 17, 17] and res[0]["event"] == (0, 3)
    # a tie at the front: the parent is the LAST in pointer order, pKFmax the first
    kfp, n_mp = shared([17, 17])
    W, res, _, _ = run_update(lib, backend, World(kfp, n_mp, order=[0, 1, 2]), [0], variants=["asc_ties"])
    assert res[0]["kfmax"] == 1 and res[0]["event"] == (0, 2)


@pytest.mark.parametrize("backend", BACKENDS)
def test_order_of_the_list_matters(lib, backend):
    """A holds each of the 10 points it shares with B twice: A counts B 20 times, B counts A 10 times.  A then B leaves weight 10 on both
    sides, B then A weight 20"""
    kfp, n_mp = shared([10], dup={0: 10})
    W1, _, _, _ = run_update(lib, backend, World(kfp, n_mp), [0, 1], variants=["count_once"])
    W2, _, _, _ = run_update(lib, backend, World(kfp, n_mp), [1, 0], variants=["count_once"])
    assert W1.kfs[0]["conn"] == {1: 10} and W1.kfs[1]["conn"] == {0: 10} and W1.kfs[0]["ow"] == [10]
    assert W2.kfs[0]["conn"] == {1: 20} and W2.kfs[1]["conn"] == {0: 20} and W2.kfs[1]["ow"] == [20]


@pytest.mark.parametrize("backend", BACKENDS)
def test_skips(lib, backend):
    """a bad point, a bad observer, an observer in another map, an observer in another slot with A's mnId; a bad key frame already in a
    neighbour's map is dropped by that neighbour's rebuild but kept by A's own list"""
    kfp, n_mp = shared([16, 16, 16, 16, 16])
    base = dict(order=[3, 1, 5, 0, 2, 4])
    W, res, _, _ = run_update(lib, backend, World(kfp, n_mp, bad_mp=range(16), **base), [0], variants=["asc_ties"])
    assert 1 not in W.kfs[0]["conn"] and res[0]["n_counter"] == 4
    W, res, _, _ = run_update(lib, backend, World(kfp, n_mp, bad_kf={2}, **base), [0], variants=["asc_ties"])
    assert 2 not in W.kfs[0]["conn"] and W.kfs[2]["conn"] == {}
    W, res, _, _ = run_update(lib, backend, World(kfp, n_mp, map_ids=[0, 0, 0, 1, 0, 0], **base), [0], variants=["asc_ties"])
    assert 3 not in W.kfs[0]["conn"]
    W, res, _, _ = run_update(lib, backend, World(kfp, n_mp, ids=[9, 1, 2, 3, 9, 5], **base), [0], variants=["asc_ties"])
    assert 4 not in W.kfs[0]["conn"] and res[0]["n_counter"] == 4
    W0 = World(kfp, n_mp, bad_kf={5}, **base)
    preload(W0, 1, [(5, 40), (2, 30)], rebuild=False)
    W0.kfs[1]["okf"], W0.kfs[1]["ow"] = [5, 2], [40, 30]   # listed before it went bad
    W, _, _, _ = run_update(lib, backend, W0, [0])
    assert W.kfs[1]["okf"] == [2, 0] and 5 in W.kfs[1]["conn"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_right_record_after_its_left(lib, backend):
    """an ORBM_OBS_RIGHT record directly after a record of the same key frame is the same entry: B counts 15, not 30"""
    kfp, n_mp = shared([15, 15])
    W, res, _, _ = run_update(lib, backend, World(kfp, n_mp, right=[(p, 1) for p in range(15)]), [0], variants=["gt"])
    assert W.kfs[0]["conn"] == {1: 15, 2: 15}


@pytest.mark.parametrize("backend", BACKENDS)
def test_init_key_frame_keeps_its_flag(lib, backend):
    kfp, n_mp = shared([14])
    W, res, _, _ = run_update(lib, backend, World(kfp, n_mp, ids=[77, 78]), [0, 1], init_id=77, variants=["own_filtered"])
    assert W.kfs[0]["first"] and W.kfs[0]["parent"] is None and [r["event"] for r in res] == [None, (1, 0)]


@pytest.mark.parametrize("backend", BACKENDS)
def test_bad_indices(lib, backend):
    """every kind: treated as absent, flagged, never read through"""
    kfp, n_mp = shared([16, 17, 3])
    mk = lambda **kw: World(kfp, n_mp, order=[2, 0, 3, 1], **kw)   # noqa: E731

    def drop_point(p):
        def f(W):
            for K in W.kfs:
                K["mp"] = [None if q == p else q for q in K["mp"]]
            W.mps[p]["obs"] = []
        return f

    def drop_record(p, k):
        def f(W):
            W.mps[p]["obs"].remove(k)
        return f
    # a list entry out of range, and one that names an empty slot
    for bad_entry in (-1, 4, 99):
        run_update(lib, backend, mk(), [0, bad_entry, 1], expect_flags=COVIS_BAD_INDEX)
    run_update(lib, backend, World(kfp + [[]], n_mp, order=[2, 0, 3, 1, 4], empty={4}), [0, 4], expect_flags=COVIS_BAD_INDEX)

    def set_kf_mp(i, val):
        def f(v, c, s, l):
            v["kf_mp"][i] = val
        return f
    for val in (-2, n_mp, 1 << 30):   # a d_kf_mp entry out of range
        run_update(lib, backend, mk(), [0], corrupt=set_kf_mp(0, val), absent=lambda W: W.kfs[0]["mp"].__setitem__(0, None),
                   expect_flags=COVIS_BAD_INDEX)

    def invalid_slot(v, c, s, l):
        v["mp"]["flags"][0] = 0
    run_update(lib, backend, mk(), [0], corrupt=invalid_slot, absent=lambda W: W.kfs[0]["mp"].__setitem__(0, None), expect_flags=COVIS_BAD_INDEX)

    def record_kf(val):   # a record's kf: point 0 is observed by key frames 0 and 1; its second record in pointer order [2, 0, 3, 1] is 1
        def f(v, c, s, l):
            v["obs"]["kf"][1] = val
        return f
    for val in (-1, 4, -(1 << 31)):
        run_update(lib, backend, mk(), [0], corrupt=record_kf(val), absent=drop_record(0, 1), expect_flags=COVIS_BAD_INDEX)

    def csr(v, c, s, l):
        v["obs_start"][1] = len(v["obs"]) + 5   # point 0's range leaves the records (and point 1's runs backwards)
    run_update(lib, backend, mk(), [0], corrupt=csr, absent=lambda W: (drop_point(0)(W), drop_point(1)(W)) and None, expect_flags=COVIS_BAD_INDEX)

    def rows(v, c, s, l):
        v["kf"]["n_feat"][0] = len(v["kf_mp"]) + 1
    run_update(lib, backend, mk(), [0], corrupt=rows, absent=lambda W: W.kfs[0].__setitem__("mp", []), expect_flags=COVIS_BAD_INDEX)

    def not_a_permutation(v, c, s, l):
        v["kf_by_order"][3] = 3   # [2, 0, 3, 3]: key frame 1 has no rank, 3 is listed twice

    def no_kf1(W):
        for m in W.mps:
            if 1 in m["obs"]:
                m["obs"].remove(1)
    run_update(lib, backend, mk(), [0], corrupt=not_a_permutation, absent=no_kf1, expect_flags=COVIS_BAD_INDEX)

    def stored_kf(val):
        def f(v, c, s, l):
            s["conn"][2]["kf"][1] = val
        return f
    for val in (-1, 4):   # a stored kf in the row of key frame 2, which A's update rebuilds: the entry is not listed
        W0 = mk()
        preload(W0, 2, [(3, 30), (1, 25)])
        W, _, _, _ = run_update(lib, backend, W0, [0], corrupt=stored_kf(val), expect_flags=COVIS_BAD_INDEX, skip_rows={2})
        assert W.kfs[2]["okf"] == [3, 1, 0]


def test_bad_index_rebuild_lists_the_rest(emu_lib):
    """the stored-kf case again, reading key frame 2's rebuilt rows: the unreadable entry is skipped, the others are in order"""
    kfp, n_mp = shared([16, 17, 3])
    W0 = World(kfp, n_mp, order=[2, 0, 3, 1])
    preload(W0, 2, [(3, 30), (1, 25)])
    view, ckf, st = flatten(W0)
    st["conn"][2]["kf"][1] = 99
    G = CovisibilityGraph(st, ckf, lib=emu_lib)
    out = G.UpdateConnections(view, np.asarray([0], np.int32), INIT_NONE)
    assert int(out["flags"][0]) == COVIS_BAD_INDEX
    assert G.GetVectorCovisibleKeyFrames(2) == [3, 0] and G.GetWeight(2, 0) == 17 and G.GetWeight(2, 1) == 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_argument_errors(lib, backend):
    kfp, n_mp = shared([16, 17])
    view, ckf, st = flatten(World(kfp, n_mp))
    dv, dckf, ds = upload(view, ckf, st, backend)
    G = CovisibilityGraph(ds, dckf, lib=lib)
    V, S = G._view(dv), G._store()
    o = sentinel_out(2, backend)
    a, p = orbhip.matcher._addr, orbhip.matcher.ptr
    lst = to_dev_plain(np.asarray([0, 1], np.int32), backend)
    work = G.Workspace(2)
    outs = lambda: CovisOut(*[a(o[k]) for k in ("child_events", "n_child_events", "nmax", "kfmax", "n_counter", "overflow_kf", "flags")])   # noqa: E731
    view_ = lambda: LocalMapView.from_buffer_copy(V)   # noqa: E731
    store_ = lambda: CovisStore.from_buffer_copy(S)    # noqa: E731

    def call(Vv=None, Ss=None, O=None, n=2, ck=dckf, kf=dv["kf"], li=lst, wk=work):
        Vv, Ss, O = Vv or view_(), Ss or store_(), O or outs()
        return lib.orbm_update_connections(C.byref(Vv), C.byref(Ss), p(ck), p(kf), p(li), n, 0, C.byref(O), p(wk), None)
    assert call() == 0 and call(n=0) == 0
    sync(backend)
    assert [call(n=-1), call(ck=None), call(kf=None), call(li=None), call(wk=None)] == [ORB_E_INVALID] * 5
    assert lib.orbm_update_connections(None, None, None, None, None, 1, 0, None, None, None) == ORB_E_INVALID
    for name in ("d_mp", "d_obs_start", "d_obs", "d_kf", "d_kf_mp", "d_kf_by_order"):
        x = view_()
        setattr(x, name, None)
        assert call(Vv=x) == ORB_E_INVALID, name
    for name in ("n_mp", "n_obs", "n_kf", "n_kf_mp_rows"):
        x = view_()
        setattr(x, name, -1)
        assert call(Vv=x) == ORB_E_INVALID, name
    for name, _ in CovisStore._fields_[:5]:
        x = store_()
        setattr(x, name, None)
        assert call(Ss=x) == ORB_E_INVALID, name
    x = store_()
    x.cap_conn = 0
    assert call(Ss=x) == ORB_E_INVALID
    x = store_()
    x.d_conn = x.d_conn + 4
    assert call(Ss=x) == ORB_E_INVALID      # a misaligned slab
    x = view_()
    x.d_mp = x.d_mp + 4
    assert call(Vv=x) == ORB_E_INVALID
    assert call(wk=work[4:]) == ORB_E_INVALID   # a misaligned workspace
    for name, _ in CovisOut._fields_:
        x = outs()
        setattr(x, name, None)
        assert call(O=x) == ORB_E_INVALID, name
    # orbm_erase_connections
    ev, n_ev = rec_dev(np.zeros(2, CULL_EVENT_DTYPE), backend), to_dev_plain(np.zeros(1, np.int32), backend)

    def erase(Vv=None, Ss=None, O=None, kf=dv["kf"], e=ev, n=n_ev, cap=2, wk=work):
        Vv, Ss, O = Vv or view_(), Ss or store_(), O or outs()
        return lib.orbm_erase_connections(C.byref(Vv), C.byref(Ss), p(kf), p(e), p(n), None, cap, C.byref(O), p(wk), None)
    assert erase() == 0 and erase(cap=0, e=None) == 0
    sync(backend)
    assert [erase(kf=None), erase(e=None), erase(n=None), erase(cap=-1), erase(wk=None), erase(wk=work[4:])] == [ORB_E_INVALID] * 6
    assert lib.orbm_erase_connections(None, None, None, None, None, None, 0, None, None, None) == ORB_E_INVALID
    x = outs()
    x.d_flags = None
    assert erase(O=x) == ORB_E_INVALID
    x = store_()
    x.cap_conn = 0
    assert erase(Ss=x) == ORB_E_INVALID
    x = view_()
    x.n_kf = -1
    assert erase(Vv=x) == ORB_E_INVALID
    assert lib.orbm_covis_workspace_bytes(-1, 1) == 0 and lib.orbm_covis_workspace_bytes(1, -1) == 0
    assert lib.orbm_covis_workspace_bytes(10, 3) >= 4 * (3 * 10 + 4 * 10) and lib.orbm_covis_workspace_bytes(10, 3) % 16 == 0
    with pytest.raises(orbhip.OrbHipError):
        G.check_flags(dict(flags=np.array([COVIS_OVERFLOW]), overflow_kf=np.array([3])))


# ------------------------------------------------------------------------------------------------ the erase
def connected_world(rng, n_kf, maps, order=None):
    """key frames without points whose weight maps are given: maps = {k: [(other, weight), ...]}"""
    W = World([[] for _ in range(n_kf)], 1, order=order, rng=rng if order is None else None)
    for k, conn in maps.items():
        preload(W, k, conn)
    return W


@pytest.mark.parametrize("backend", BACKENDS)
def test_erase_stamp(lib, backend):
    """B.map holds K1 and K2; K2.map lacks B, so only K1's event rebuilds B: K2, erased by the LATER event, stays in B's list.  Filtering by
    the final bad flags drops it"""
    maps = {0: [(1, 20), (2, 30), (3, 16)], 1: [(0, 20)], 2: [(3, 40)], 3: [(2, 40), (0, 16)]}
    for flag_bad in (False, True):
        W, _ = run_erase(lib, backend, connected_world(None, 4, maps, order=[0, 1, 2, 3]), [(1, True), (2, True)], flag_bad=flag_bad,
                         variants=["final_bad"])
        assert W.kfs[0]["conn"] == {2: 30, 3: 16} and W.kfs[0]["okf"] == [2, 3] and W.stats["stamp_kept"] >= 1
        assert W.kfs[3]["conn"] == {0: 16} and W.kfs[3]["okf"] == [0] and W.kfs[1]["conn"] == {} == W.kfs[2]["conn"]
    # the other order: K2's event changes nothing of B, K1's comes later and sees K2 bad
    W, _ = run_erase(lib, backend, connected_world(None, 4, maps, order=[0, 1, 2, 3]), [(2, True), (1, True)])
    assert W.kfs[0]["conn"] == {2: 30, 3: 16} and W.kfs[0]["okf"] == [3]


@pytest.mark.parametrize("backend", BACKENDS)
def test_erase_deferred_absent_and_cleared(lib, backend):
    """a deferred event is skipped; the erased key frame's row and list are emptied; an erase of an absent entry rebuilds nothing (a stale
    list stays); d_kf_erased = NULL takes every event"""
    maps = {0: [(1, 20), (2, 18)], 1: [(0, 20), (2, 5), (3, 17)], 2: [(0, 18), (1, 5)], 3: [(0, 9)]}
    W0 = connected_world(None, 4, maps, order=[3, 1, 0, 2])
    W0.kfs[3]["okf"], W0.kfs[3]["ow"] = [0, 2], [9, 1]   # stale on purpose: key frame 1 names 3, whose map has no entry of 1
    W, _ = run_erase(lib, backend, W0, [(2, False), (1, True)])
    assert W.kfs[2]["conn"] == {0: 18} and W.kfs[1]["conn"] == {} and W.kfs[1]["okf"] == []
    assert W.kfs[0]["conn"] == {2: 18} and W.kfs[3]["okf"] == [0, 2] and 3 not in W.rebuilt
    W, _ = run_erase(lib, backend, W0, [(2, False), (1, True)], pass_erased=False)
    assert W.kfs[2]["conn"] == {} and W.kfs[0]["conn"] == {}
    run_erase(lib, backend, W0, [])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n_row", [1, 63, 64, 65, 130])
def test_erase_row_lengths(lib, backend, n_row):
    """the erased entry at the front, in the middle and at the end of rows of n_row entries: the entries behind move up, in order"""
    rng = np.random.default_rng(200 + n_row)
    n_kf = n_row + 4
    others = [(k, 1 + int(rng.integers(0, 50))) for k in range(4, 4 + n_row - 1)]
    maps = {0: [(3, 21)] + others, 1: others[:n_row // 2] + [(3, 22)] + others[n_row // 2:], 2: others + [(3, 23)], 3: [(0, 21), (1, 22), (2, 23)]}
    W0 = connected_world(rng, n_kf, maps)
    W0.cap_conn = max(n_row, 3)
    W, _ = run_erase(lib, backend, W0, [(3, True)])
    assert all(list(W.kfs[k]["conn"].items()) == others for k in (0, 1, 2)) and len(W.kfs[0]["okf"]) == n_row - 1


@pytest.mark.parametrize("backend", BACKENDS)
def test_erase_same_before_and_after_apply(lib, backend):
    """the same events on a view that already carries ORBM_LM_KF_BAD for them (the call after orbm_apply_keyframe_culling): the same store"""
    rng = np.random.default_rng(11)
    W0 = fuzz_world(rng, 20, 200, 60)
    update_all(W0, list(rng.permutation(20)))
    events = [(int(k), bool(rng.random() < 0.8)) for k in rng.permutation(20)[:8]]
    _, before = run_erase(lib, backend, copy.deepcopy(W0), events)
    _, after = run_erase(lib, backend, copy.deepcopy(W0), events, flag_bad=True)
    for k in before:
        assert np.array_equal(before[k], after[k]), k


@pytest.mark.parametrize("backend", BACKENDS)
def test_erase_bad_indices(lib, backend):
    maps = {0: [(1, 20), (2, 18)], 1: [(0, 20)], 2: [(0, 18)]}
    mk = lambda: connected_world(None, 3, maps, order=[0, 1, 2])   # noqa: E731
    W0 = mk()   # an event's key frame out of range: skipped
    view, ckf, st = flatten(W0)
    ev = np.zeros(3, CULL_EVENT_DTYPE)
    ev["kf"] = [7, 2, -5]
    dv, dckf, ds = upload(view, ckf, st, backend)
    G = CovisibilityGraph(ds, dckf, lib=lib)
    out = G.EraseConnections(dv, rec_dev(ev, backend), to_dev_plain(np.asarray([3], np.int32), backend))
    sync(backend)
    assert int(to_host(out["flags"])[0]) == COVIS_BAD_INDEX
    W = copy.deepcopy(W0)
    erase_connections(W, [(2, True)])
    check_store(W, view, ckf, st, dv, dckf, ds)
    # a count beyond cap_events is clamped and flagged; a stored kf out of range in the erased row is skipped
    for n_ev, stored in ((9, None), (1, 5)):
        W0 = mk()
        view, ckf, st = flatten(W0)
        if stored is not None:
            st["conn"][0]["kf"][0] = stored
        dv, dckf, ds = upload(view, ckf, st, backend)
        G = CovisibilityGraph(ds, dckf, lib=lib)
        ev = np.zeros(1, CULL_EVENT_DTYPE)
        out = G.EraseConnections(dv, rec_dev(ev, backend), to_dev_plain(np.asarray([n_ev], np.int32), backend))
        sync(backend)
        assert int(to_host(out["flags"])[0]) == COVIS_BAD_INDEX
        got = to_host(ds["n_conn"])
        assert list(got) == ([0, 0, 0] if stored is None else [0, 1, 0])


# ------------------------------------------------------------------------------------------------ the chains
def as_rec(a, dtype):
    a = to_host(a)
    return a.copy() if a.dtype.names else np.ascontiguousarray(a).view(dtype).reshape(a.shape[:-1]).copy()


def local_map(m, backend, view, votes, out=None, d_vote=None, cap_kf=32):
    """orbm_update_local_map of one frame that holds `votes` on `view` -> (the library's dict, the vote arrays with the frame record)"""
    n_mp = int(view["mp"].shape[0])
    if d_vote is None:
        a = np.full((1, len(votes) + 3), -1, np.int32)
        a[0, :len(votes)] = votes
        fr = np.zeros(1, LOCALMAP_FRAME_DTYPE)
        fr["last_kf"] = -1
        d_vote = (to_dev_plain(a, backend), to_dev_plain(np.asarray([len(votes)], np.int32), backend), to_dev(fr, backend))
    return m.UpdateLocalMap(view, d_vote[2], d_vote[0], d_vote[1], d_vote[0], d_vote[1], cap_kf, n_mp, out=out), d_vote


def local_map_result(m, out):
    m.check_local_map(out)
    nk, nm = int(to_host(out["n_local_kf"])[0]), int(to_host(out["nmp"])[0])
    return [to_host(out["local_kf"])[0, :nk].copy(), to_host(out["local_src"])[0, :nm].copy(), np.asarray([int(to_host(out["ref_kf"])[0]), nk, nm]),
            to_host(out["local_mp"])[0, :nm].copy()]


def with_local_map_arrays(view, backend):
    """the view with the members orbm_update_local_map reads beyond the graph's: no children, a zeroed track slab"""
    n_mp = int(view["mp"].shape[0])
    return dict(view, children=to_dev_plain(np.zeros(0, np.int32), backend), mp_track=rec_dev(np.zeros(n_mp, TRACK_DTYPE), backend))


class AppendChain:
    """create -> append -> refresh -> update connections -> update local map on the batch of tests/test_new_map_points.py append_cases():
    key frame 0 is the current one (kf1 of every pair), key frames 1..5 its neighbours; 37 older points with three observers each."""
    ROW = 340   # features per key frame, padded with NULL: the slabs keep their shape whatever the matches give

    def __init__(self, lib, backend):
        import test_new_map_points as tnp
        self.tnp, self.lib, self.backend = tnp, lib, backend
        self.cases, _ = tnp.append_cases()
        for c in self.cases[1:]:
            c["P"]["cam1"]["Ow"] = self.cases[0]["P"]["cam1"]["Ow"]
        self.s1, self.s2, self.pairs, self.m12 = tnp.batch_arrays(self.cases)
        self.n_kf = len(self.cases) + 1
        self.m = orbhip.ORBmatcher(lib=lib)
        self.d1, self.d2 = tnp.upload_side(self.s1, backend), tnp.upload_side(self.s2, backend)
        self.dp, self.dm = to_dev(self.pairs, backend), to_dev_plain(self.m12.copy(), backend)
        self.has0 = [to_host(self.d1["has_mp"]).copy(), to_host(self.d2["has_mp"]).copy()]
        self.kf_c, self.kf_desc = tnp.refresh_world(self.cases, None)
        self.d_kfc, self.d_kfd = to_dev(self.kf_c, backend), to_dev_plain(self.kf_desc, backend)
        self.prm = self.m.RefreshParams(tnp.SF)
        self.dev, self.out = {}, {}

    def world(self, m12):
        """the restated create + append for these matches -> (before, after, the World with its graph before the update)"""
        tnp, cur = self.tnp, 37
        created = [tnp.restate_pair(self.pairs[b], tnp.host_side(self.s1, b), tnp.host_side(self.s2, b), m12[b], 120) for b in range(len(self.cases))]
        before, after = tnp.append_world(self.cases, created, **tnp.APPEND_ROOMY)
        for x in (before, after):
            for p in range(cur):
                for j in range(3):
                    x["obs"][3 * p + j] = ((p + 2 * j) % self.n_kf, 0, 0)
            x["mp"]["flags"][:cur] = MP_VALID
        before["mp"]["flags"][cur:] = 0
        n_final = int(after["n_mp"][0])
        after["mp"]["flags"][n_final:] = 0
        rows = [[] for _ in range(self.n_kf)]
        for p in range(n_final):
            for o in range(after["obs_start"][p], after["obs_start"][p + 1]):
                rows[int(after["obs"][o]["kf"])].append(p)
        rows[0] += rows[0][:10]   # the current key frame holds ten of its points twice
        assert max(len(r) for r in rows) <= self.ROW
        W = World([r + [None] * (self.ROW - len(r)) for r in rows], 400, order=[4, 1, 0, 5, 3, 2], cap_conn=self.n_kf + 1)
        for k in (1, 2, 3):   # the neighbours met before: stale weights, one of them below the threshold
            preload(W, k, [((k + 1) % self.n_kf or 1, 3 + k), (0, 2)])
        return before, after, W

    def load(self, m12):
        """the device state before the chain; -> (after, the World, the host arrays of the graph and the key-frame slabs)"""
        tnp, bk = self.tnp, self.backend
        before, after, W = self.world(m12)
        view_w, ckf, st = flatten(W)
        host = dict(mp=before["mp"], obs=before["obs"], ref=before["ref"], obs_start=before["obs_start"], n_mp=before["n_mp"],
                    desc=np.full((400, 32), SENT8, np.uint8), sel=before["sel"], kf=view_w["kf"], kf_mp=view_w["kf_mp"],
                    kf_by_order=view_w["kf_by_order"], ckf=ckf, m12=m12, has1=self.has0[0], has2=self.has0[1], **{"st_" + k: v for k, v in st.items()})
        for k, v in host.items():
            t = rec_dev(v, bk) if v.dtype.names else to_dev_plain(v.copy(), bk)
            if k not in self.dev:
                self.dev[k] = t
            elif bk == "hip":
                self.dev[k].copy_(t)
            else:
                self.dev[k][...] = t
        if "appended" not in self.dev:
            self.dev["appended"] = to_dev_plain(np.zeros(2, np.int32), bk)
            self.dev["track"] = rec_dev(np.zeros(400, TRACK_DTYPE), bk)
            self.dev["children"] = to_dev_plain(np.zeros(0, np.int32), bk)
            self.dev["list"] = to_dev_plain(np.asarray([0], np.int32), bk)
            votes = np.full((1, 44), -1, np.int32)
            votes[0, :40] = np.arange(0, 80, 2)   # points that every variant of the matches leaves valid
            fr = np.zeros(1, LOCALMAP_FRAME_DTYPE)
            fr["last_kf"] = -1
            self.dev["vote"] = (to_dev_plain(votes, bk), to_dev_plain(np.asarray([40], np.int32), bk), to_dev(fr, bk))
            self.votes0 = votes
        D = self.dev
        if bk == "hip":
            D["vote"][0].copy_(to_dev_plain(self.votes0, bk))
        else:
            D["vote"][0][...] = self.votes0
        self.d1["has_mp"], self.d2["has_mp"], self.dm = D["has1"], D["has2"], D["m12"]
        self.view = dict(mp=D["mp"], obs_start=D["obs_start"], obs=D["obs"], kf=D["kf"], kf_mp=D["kf_mp"], kf_by_order=D["kf_by_order"],
                         children=D["children"], mp_track=D["track"])
        self.G = CovisibilityGraph({k: D["st_" + k] for k in st}, D["ckf"], lib=self.lib)
        return after, W, view_w, ckf, st

    def step(self):
        m, D, o = self.m, self.dev, self.out
        o["created"] = m.CreateNewMapPoints(self.d1, self.d2, self.dp, self.dm, 120, out=o.get("created"))
        m.AppendNewMapPoints(o["created"], self.dp, self.d1["kps"], D["n_mp"], D["mp"], 400, D["obs_start"], D["obs"], D["ref"], 300,
                             out=dict(sel=D["sel"], appended=D["appended"]))
        o["res"] = m.RefreshMapPoints(D["mp"], D["desc"], D["obs_start"], D["obs"], D["ref"], self.d_kfc, self.d_kfd, self.prm, sel=D["sel"],
                                      out=o.get("res"))
        o["covis"] = self.G.UpdateConnections(self.view, D["list"], INIT_NONE, out=o.get("covis"))
        o["local"], _ = local_map(m, self.backend, self.view, None, out=o.get("local"), d_vote=D["vote"])

    def snapshot(self):
        sync(self.backend)
        D = self.dev
        return [to_host(D[k]).copy() for k in ("st_conn", "st_n_conn", "st_ordered_kf", "st_ordered_w", "st_n_ordered", "kf", "ckf", "n_mp")] + \
            [to_host(self.out["covis"][k]).copy() for k in ("nmax", "kfmax", "n_counter", "flags", "n_child_events")] + local_map_result(self.m, self.out["local"])


@pytest.mark.parametrize("backend", BACKENDS)
def test_chain_create_append_refresh_update(lib, backend):
    """create -> append -> refresh -> update connections -> orbm_update_local_map with no host step in between: the graph is the restatement's
    on the restated map, and the local map equals that of the existing path fed with the restatement's covis[] and parent"""
    ch = AppendChain(lib, backend)
    after, W, view_w, ckf, st = ch.load(ch.m12)
    ch.step()
    sync(backend)
    D = ch.dev
    assert int(to_host(D["n_mp"])[0]) == int(after["n_mp"][0]) > 150 and np.array_equal(to_host(D["obs_start"]), after["obs_start"])
    res = update_connections(W, 0, INIT_NONE)
    assert res["n_counter"] == 5 and res["nmax"] >= TH and W.stats["sub_listed"] >= 1
    o = ch.out["covis"]
    assert [int(to_host(o[k])[0]) for k in ("nmax", "kfmax", "n_counter", "flags", "n_child_events")] == [res["nmax"], res["kfmax"], 5, 0, 1]
    view0 = dict(view_w, mp=as_rec(D["mp"], MAP_POINT_DTYPE), obs_start=to_host(D["obs_start"]).copy(), obs=to_host(D["obs"]).copy())
    check_store(W, view0, ckf, st, ch.view, D["ckf"], ch.G.store)
    got = local_map_result(ch.m, ch.out["local"])
    host_view = dict(ch.view, kf=rec_dev(flatten(W)[0]["kf"], backend), mp_track=rec_dev(np.zeros(400, TRACK_DTYPE), backend))
    want, _ = local_map(ch.m, backend, host_view, list(range(0, 80, 2)))
    sync(backend)
    want = local_map_result(ch.m, want)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and got[2][1] >= 4 and got[2][2] > 150

@pytest.mark.gpu
def test_chain_graph_capture_replay_hip(hip_lib):
    """the first chain captured once on a single stream and replayed twice on changed matches == the eager calls"""
    import torch
    ch = AppendChain(hip_lib, "hip")
    rng = np.random.default_rng(1300)
    inputs = []
    for it in range(2):
        m12 = ch.m12.copy()
        m12[rng.random(m12.shape) < 0.3 + 0.2 * it] = -1
        inputs.append(m12)
    eager = []
    for m12 in inputs:
        ch.load(m12)
        ch.step()
        eager.append(ch.snapshot())
    assert int(eager[0][7][0]) != int(eager[1][7][0]) and min(int(e[7][0]) for e in eager) > 80
    ch.load(inputs[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ch.step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    ch.load(inputs[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ch.step()
    for r, (m12, want) in enumerate(zip(inputs, eager)):
        ch.load(m12)
        torch.cuda.synchronize()
        g.replay()
        got = ch.snapshot()
        for i, (x, y) in enumerate(zip(got, want)):
            assert np.array_equal(x, y), (r, i)


@pytest.mark.parametrize("backend", BACKENDS)
def test_chain_cull_apply_erase(lib, backend):
    """cull -> apply -> erase -> orbm_update_local_map: the events, their count and the erased bytes are read where orbm_cull_keyframes left
    them; the graph is the restatement's, the local map that of the existing path fed with the restatement's covis[]"""
    rng = np.random.default_rng(31)
    n_kf, nf = 9, 40
    rows = [list(range(nf)) + [nf + 3 * k + i for i in range(3)] for k in range(n_kf)]   # 40 shared points, 3 of its own: 40 of 43 redundant
    W = World(rows, nf + 3 * n_kf, rng=rng)
    update_all(W, [int(k) for k in rng.permutation(n_kf)])
    W.stats = dict(unchanged=0, sub_listed=0, stamp_kept=0, none15=0)
    view, ckf, st = flatten(W)
    dv, dckf, ds = upload(view, ckf, st, backend)
    G = CovisibilityGraph(ds, dckf, lib=lib)
    m = orbhip.ORBmatcher(lib=lib)
    cur = n_kf - 1
    cands = W.kfs[cur]["okf"]
    assert len(cands) == n_kf - 1
    cull_ckf, feat = flatten_cull_keyframes([dict(mp=[-1 if p is None else p for p in K["mp"]], id=K["id"]) for K in W.kfs])
    cull = dict(ckf=rec_dev(cull_ckf, backend), feat=to_dev_plain(feat, backend), mp_nobs=None)
    pr = np.zeros(1, CULL_PROBLEM_DTYPE)
    pr[0] = (cur, INIT_NONE, 0, len(cands), n_kf, CULL_MONOCULAR)
    culled = m.CullKeyFrames(dv, cull, rec_dev(pr, backend), to_dev_plain(np.asarray(cands, np.int32), backend), len(cands) + 2, n_cand_max=len(cands))
    m.check_cull_flags(culled)
    ref = rec_dev(np.zeros(len(W.mps), REFRESH_POINT_DTYPE), backend)
    app = m.ApplyKeyFrameCulling(dv, cull, culled, ref, len(view["obs"]))
    m.check_cull_applied(app)
    sync(backend)
    n_ev = int(to_host(culled["n_events"])[0])
    events = [(int(k), True) for k in as_rec(culled["events"], CULL_EVENT_DTYPE)[0, :n_ev]["kf"]]
    assert n_ev >= 3 and [k for k, _ in events] == cands[:n_ev]
    view0 = {k: (as_rec(v, {"mp": MAP_POINT_DTYPE, "kf": LOCALMAP_KEYFRAME_DTYPE, "obs": view["obs"].dtype}[k]) if k in ("mp", "kf", "obs")
                 else to_host(v).copy()) for k, v in dv.items()}
    assert all(view0["kf"]["flags"][k] & LM_KF_BAD for k, _ in events)
    out = G.EraseConnections(dv, culled=culled, problem=0)
    sync(backend)
    assert int(to_host(out["flags"])[0]) == 0
    erase_connections(W, events)
    assert W.stats["stamp_kept"] >= 1
    check_store(W, view0, ckf, st, dv, dckf, ds)
    # the local map on the applied map: the device's key-frame slab against one built from the restatement
    applied = with_local_map_arrays(dict(dv, obs_start=app["obs_start"], obs=app["obs"]), backend)
    got, _ = local_map(m, backend, applied, list(range(0, len(W.mps), 2)))
    kf = view0["kf"].copy()
    for k, K in enumerate(W.kfs):
        kf[k]["covis"] = (K["okf"][:10] + [-1] * 10)[:10]
    want, _ = local_map(m, backend, with_local_map_arrays(dict(applied, kf=rec_dev(kf, backend)), backend), list(range(0, len(W.mps), 2)))
    sync(backend)
    got, want = local_map_result(m, got), local_map_result(m, want)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and got[2][1] >= n_kf - n_ev



# ------------------------------------------------------------------------------------------------ getters
def test_getters(emu_lib):
    kfp, n_mp = shared([17, 17, 18, 16, 3])
    W0 = World(kfp, n_mp, order=[4, 2, 0, 5, 1, 3])
    view, ckf, st = flatten(W0)
    G = CovisibilityGraph(st, ckf, lib=emu_lib)
    G.UpdateConnections(view, np.asarray([0], np.int32), INIT_NONE)
    assert G.GetVectorCovisibleKeyFrames(0) == [3, 1, 2, 4] and G.GetBestCovisibilityKeyFrames(0, 2) == [3, 1]
    assert G.GetBestCovisibilityKeyFrames(0, 10) == [3, 1, 2, 4] and G.GetWeight(0, 5) == 3 and G.GetWeight(0, 0) == 0 and G.GetWeight(3, 0) == 18
    assert G.GetCovisiblesByWeight(0, 17) == [3, 1, 2] and G.GetCovisiblesByWeight(0, 18) == [3] and G.GetCovisiblesByWeight(0, 19) == []
    assert G.GetCovisiblesByWeight(0, 1) == [3, 1, 2, 4] and G.GetCovisiblesByWeight(5, 1) == []


# ------------------------------------------------------------------------------------------------ fuzz
def fuzz_world(rng, n_kf, n_mp, n_feat):
    kfp = []
    for _ in range(n_kf):
        nf = int(rng.integers(0, n_feat + 1))
        lo = int(rng.integers(0, max(n_mp - 40, 1)))
        pts = [int(p) for p in rng.integers(lo, min(lo + 60, n_mp), nf)]          # neighbours in a window share many points; duplicates happen
        kfp.append([None if rng.random() < 0.15 else p for p in pts])
    ids = list(range(100, 100 + n_kf))
    if n_kf > 3 and rng.random() < 0.5:
        ids[1] = ids[0]
    W = World(kfp, n_mp, rng=rng, bad_kf={int(k) for k in rng.permutation(n_kf)[:int(rng.integers(0, 3))]},
              bad_mp={int(p) for p in rng.integers(0, n_mp, 5)}, ids=ids, map_ids=[0 if rng.random() < 0.9 else 1 for _ in range(n_kf)],
              right=[(int(p), int(k)) for p in range(n_mp) for k in range(n_kf) if rng.random() < 0.02], cap_conn=n_kf + 1)
    for p, k in list((p, k) for p in range(n_mp) for k in W.mps[p]["right"]):
        if k not in W.mps[p]["obs"]:
            W.mps[p]["right"].discard(k)
    return W


def update_all(W, order):
    for a in order:
        update_connections(W, int(a), W.kfs[0]["id"])
    W.rebuilt = set()


FUZZ_SEEDS = list(range(24))


def fuzz_case(seed):
    """-> (the world after a first round of updates in random order, the list to update, the erase events)"""
    rng = np.random.default_rng(1000 + seed)
    n_kf = int(rng.integers(3, 41))
    W = fuzz_world(rng, n_kf, int(rng.integers(30, 300)), int(rng.integers(1, 81)))
    update_all(W, [int(k) for k in rng.permutation(n_kf)[:int(rng.integers(0, n_kf + 1))]])
    # the map moves on: some points are dropped from some key frames, so that counts fall and weights go stale
    for k, K in enumerate(W.kfs):
        if rng.random() < 0.5:
            for i, p in enumerate(K["mp"]):
                if p is not None and rng.random() < 0.3:
                    K["mp"][i] = None
                    if p not in K["mp"] and k in W.mps[p]["obs"]:
                        W.mps[p]["obs"].remove(k)
                        W.mps[p]["right"].discard(k)
    lst = [int(k) for k in rng.integers(0, n_kf, int(rng.integers(1, 13)))]
    events = [(int(k), bool(rng.random() < 0.85)) for k in rng.permutation(n_kf)[:int(rng.integers(1, max(n_kf // 2, 2)))]]
    W.stats = dict(unchanged=0, sub_listed=0, stamp_kept=0, none15=0)
    return W, lst, events


def test_fuzz_seeds_are_not_vacuous():
    """from the restatement alone: over the seed set, an unchanged-weight return, a sub-threshold entry listed by a rebuild, a bad key frame
    kept in a list by the stamp rule, a call in which no one reaches 15"""
    tot = dict(unchanged=0, sub_listed=0, stamp_kept=0, none15=0)
    differs = 0
    for seed in FUZZ_SEEDS:
        W, lst, events = fuzz_case(seed)
        init = W.kfs[0]["id"]
        for a in lst:
            update_connections(W, a, init)
        X = copy.deepcopy(W)
        erase_connections(W, events)
        erase_connections(X, events, variant="final_bad")
        differs += state(X) != state(W)
        for k in tot:
            tot[k] += W.stats[k]
    assert all(v > 0 for v in tot.values()) and differs > 0, (tot, differs)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz(lib, backend, seed):
    W0, lst, events = fuzz_case(seed)
    W, _, _, _ = run_update(lib, backend, W0, lst, init_id=W0.kfs[0]["id"])
    W.rebuilt, W.raw = set(), None
    run_erase(lib, backend, W, events)


def test_reversed_lane_order():
    """the emulated build under EMU_REVERSE=1 (lanes scheduled in reverse): nothing depends on the order of the lanes"""
    env = dict(os.environ, EMU_REVERSE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", __file__, "-k",
                        "emu and not reversed and not chain and (fuzz or erase or row or threshold or nobody or equal or order_of or key_frame_counts)"],
                       env=env, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
