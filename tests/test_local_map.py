"""Tracking::UpdateLocalMap on the device map (include/orbhip.h "Local map"): orbm_update_local_map and orbm_store_local_tracks against a literal
Python restatement of Tracking::UpdateLocalKeyFrames (Tracking.cc:3042-3244), Tracking::UpdateLocalPoints (:2998-3036) and the marking loop
of Tracking::SearchLocalPoints (:2852-2872).  Integer work: every output array is compared bit for bit, the bytes past the counts against a
sentinel."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import orbhip
import test_map_projection as tmp
from devarrays import BACKENDS, lib, to_dev, to_dev_plain, to_host  # noqa: F401
from orbhip._abi import (LM_BAD_INDEX, LM_INERTIAL, LM_KF_OVERFLOW, LM_MP_OVERFLOW, LOCALMAP_FRAME_DTYPE, MAP_POINT_DTYPE, MP_BAD, MP_HAS_OBS,
                         MP_SEEN, MP_VALID, OBS_RIGHT, ORB_E_INVALID, PROJ_LOCAL_MAP, QUERY_DTYPE, TRACK_DTYPE, LocalMapLists, LocalMapOut,
                         LocalMapView)
from orbhip.matcher import flatten_local_map_keyframes, flatten_observations

SENT8 = 0x5A
SENT32 = 0x5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ a flattened map
class World:
    """kfs: per slot None or dict(bad, parent, prev, mp, covis, children); mp_flags uint32 [n_mp]; obs: per point [(kf, flags)] in
    mObservations order; order: the key-frame index at each rank of pointer order"""

    def __init__(self, rng, kfs, mp_flags, obs, order=None, B=1):
        self.kfs, self.n_kf, self.n_mp = kfs, len(kfs), len(mp_flags)
        self.kf, self.kf_mp, self.children = flatten_local_map_keyframes(kfs)
        self.mp = rng.integers(0, 256, (self.n_mp, MAP_POINT_DTYPE.itemsize), dtype=np.uint8).view(MAP_POINT_DTYPE)[:, 0].copy()
        self.mp["flags"] = mp_flags
        self.obs_start, self.obs = flatten_observations([[(k, 0, f) for k, f in o] for o in obs])
        self.order = np.asarray(order if order is not None else rng.permutation(self.n_kf), np.int32)
        self.track = rng.integers(0, 256, (B, self.n_mp, TRACK_DTYPE.itemsize), dtype=np.uint8).view(TRACK_DTYPE)[:, :, 0].copy()
        self.track["in_view"] = rng.integers(0, 2, (B, self.n_mp))

    def view(self, backend, track=None):
        trk = self.track if track is None else track

        def rec(a):   # an empty record array keeps its count of 0 (its pointer may be null)
            if backend == "hip" and a.size == 0:
                import torch
                return torch.zeros((0, a.dtype.itemsize), dtype=torch.uint8, device="cuda")
            return to_dev(a, backend)
        v = dict(mp=rec(self.mp), obs_start=to_dev_plain(self.obs_start, backend), obs=rec(self.obs),
                 kf=rec(self.kf), kf_mp=to_dev_plain(self.kf_mp, backend), children=to_dev_plain(self.children, backend),
                 kf_by_order=to_dev_plain(self.order, backend), mp_track=to_dev(trk if trk.shape[0] > 1 else trk[0], backend))
        if backend == "emu":
            v["mp_track"] = v["mp_track"].copy()
        return v


def random_world(rng, n_kf, n_mp, n_feat, B=1, p_bad_kf=0.05, p_bad_mp=0.05, p_empty=0.3, p_right=0.2, n_tree=True):
    """a random map whose observations agree with the key frames' features; mObservations iterates in pointer order"""
    order = rng.permutation(n_kf)
    rank = np.empty(n_kf, np.int64)
    rank[order] = np.arange(n_kf)
    fl = np.full(n_mp, MP_VALID | MP_HAS_OBS, np.uint32)
    fl[rng.random(n_mp) < p_bad_mp] |= MP_BAD
    seen_in = [[] for _ in range(n_mp)]
    kfs = []
    for k in range(n_kf):
        nf = int(rng.integers(max(n_feat // 2, 1), n_feat + 1))
        # a key frame sees a window of the map, so that neighbours share points
        lo = int(rng.integers(0, max(n_mp - 2 * nf, 1)))
        mp = rng.integers(lo, min(lo + 2 * nf, n_mp), nf)
        mp[rng.random(nf) < p_empty] = -1
        for p in set(int(x) for x in mp if x >= 0):
            seen_in[p].append(k)
        kfs.append(dict(bad=bool(rng.random() < p_bad_kf), parent=int(rng.integers(0, k)) if (k and n_tree) else -1,
                        prev=k - 1 if k else -1, mp=[int(x) for x in mp],
                        covis=[int(x) for x in rng.choice(n_kf, int(rng.integers(0, min(n_kf, 10) + 1)), replace=False) if x != k], children=[]))
    for k, d in enumerate(kfs):
        if d["parent"] >= 0:
            kfs[d["parent"]]["children"].append(k)
    for d in kfs:
        d["children"].sort(key=lambda c: rank[c])
    obs = []
    for p in range(n_mp):
        o = []
        for k in sorted(seen_in[p], key=lambda c: rank[c]):
            o.append((k, 0))
            if rng.random() < p_right:
                o.append((k, OBS_RIGHT))
        obs.append(o)
    return World(rng, kfs, fl, obs, order, B)


# ------------------------------------------------------------------------------------------------ the reference, restated
def ref_update_local_map(W, frame, vote, flist, dropped, cap_kf, cap_mp, track):
    """One frame.  vote / flist: lists, changed in place (the same object where the current frame votes).  -> dict of the outputs."""
    flags = 0
    n_mp, n_kf, n_obs = W.n_mp, W.n_kf, len(W.obs)
    kf, mpf = W.kf, W.mp["flags"]
    rank_of = {int(k): r for r, k in enumerate(W.order)}

    def point_ok(p):
        return 0 <= p < n_mp and bool(mpf[p] & MP_VALID)

    def present(v):
        return 0 <= v < n_kf and bool(kf[v]["flags"] & 1)

    def is_bad(v):
        return bool(kf[v]["flags"] & 2)

    # ---- UpdateLocalKeyFrames: the votes (:3050-3112)
    keyframeCounter = {}
    for i, p in enumerate(vote):
        if p == -1:
            continue
        if not point_ok(p):
            vote[i] = -1
            flags |= LM_BAD_INDEX
            continue
        if mpf[p] & MP_BAD:
            vote[i] = -1
            continue
        s, e = int(W.obs_start[p]), int(W.obs_start[p + 1])
        if s < 0 or e < s or e > n_obs:
            flags |= LM_BAD_INDEX
            continue
        for o in range(s, e):
            k = int(W.obs[o]["kf"])
            if (W.obs[o]["flags"] & OBS_RIGHT) and o > s and int(W.obs[o - 1]["kf"]) == k:
                continue
            if not 0 <= k < n_kf:
                flags |= LM_BAD_INDEX
                continue
            keyframeCounter[rank_of[k]] = keyframeCounter.get(rank_of[k], 0) + 1
    # ---- first level (:3131-3150)
    mx, pKFmax = 0, -1
    local, listed = [], set()
    for r in sorted(keyframeCounter):
        k = int(W.order[r])
        if not present(k):
            flags |= LM_BAD_INDEX
            continue
        if is_bad(k):
            continue
        if keyframeCounter[r] > mx:
            mx, pKFmax = keyframeCounter[r], k
        local.append(k)
        listed.add(k)
    # ---- second loop (:3155-3213)
    for i in range(len(local)):
        if len(local) > 80:
            break
        K = kf[local[i]]
        for v in K["covis"]:
            v = int(v)
            if v == -1:
                continue
            if not present(v):
                flags |= LM_BAD_INDEX
                continue
            if not is_bad(v) and v not in listed:
                local.append(v)
                listed.add(v)
                break
        cs, nc = int(K["child_start"]), int(K["n_child"])
        if nc < 0 or cs < 0 or nc > len(W.children) - cs:
            flags |= LM_BAD_INDEX
        else:
            for v in W.children[cs:cs + nc]:
                v = int(v)
                if not present(v):
                    flags |= LM_BAD_INDEX
                    continue
                if not is_bad(v) and v not in listed:
                    local.append(v)
                    listed.add(v)
                    break
        par = int(K["parent"])
        if par != -1:
            if not present(par):
                flags |= LM_BAD_INDEX
            elif par not in listed:
                local.append(par)
                listed.add(par)
                break
    # ---- inertial tail (:3217-3236)
    if (int(frame["flags"]) & LM_INERTIAL) and len(local) < 80:
        t = int(frame["last_kf"])
        for _ in range(20):
            if t == -1:
                break
            if not present(t):
                flags |= LM_BAD_INDEX
                break
            if t not in listed:
                local.append(t)
                listed.add(t)
                t = int(kf[t]["prev"])
    out = dict(local_kf=local[:cap_kf], n_local_kf=min(len(local), cap_kf), n_local_kf_required=len(local), ref_kf=pKFmax, max_votes=mx,
               local_src=[], nmp=0, nmp_required=0, all_src=[])
    # ---- the marking loop of SearchLocalPoints (:2852-2872) and the dropped points
    seen, dropped_set = set(), set()
    for i, p in enumerate(flist):
        if p == -1:
            continue
        if not point_ok(p):
            flist[i] = -1
            flags |= LM_BAD_INDEX
        elif mpf[p] & MP_BAD:
            flist[i] = -1
        else:
            seen.add(p)
    for p in dropped or ():
        if p == -1:
            continue
        if not point_ok(p):
            flags |= LM_BAD_INDEX
        else:
            dropped_set.add(p)
    if len(local) > cap_kf:
        out["flags"] = flags | LM_KF_OVERFLOW
        return out
    # ---- UpdateLocalPoints (:2998-3036)
    pts, ref_for_frame = [], set()
    for k in reversed(local):
        r0, nf = int(kf[k]["mp_row0"]), int(kf[k]["n_feat"])
        if r0 < 0 or nf < 0 or nf > len(W.kf_mp) - r0:
            flags |= LM_BAD_INDEX
            continue
        for p in W.kf_mp[r0:r0 + nf]:
            p = int(p)
            if p == -1:
                continue
            if not point_ok(p):
                flags |= LM_BAD_INDEX
                continue
            if p in ref_for_frame:
                continue
            if not mpf[p] & MP_BAD:
                pts.append(p)
                ref_for_frame.add(p)
    if len(pts) > cap_mp:
        flags |= LM_MP_OVERFLOW
    out.update(all_src=pts, local_src=pts[:cap_mp], nmp=min(len(pts), cap_mp), nmp_required=len(pts), flags=flags)
    rec = W.mp[out["local_src"]].copy() if out["nmp"] else np.zeros(0, MAP_POINT_DTYPE)
    trk = track[out["local_src"]].copy() if out["nmp"] else np.zeros(0, TRACK_DTYPE)
    for j, p in enumerate(out["local_src"]):
        if p in seen or p in dropped_set:
            rec[j]["flags"] |= MP_SEEN
        if p in dropped_set:
            trk[j]["in_view"] = 0   # NOT for the points of the frame list: the marking loop clears mbTrackInViewR (:2869)
    out["local_mp"], out["track"] = rec, trk
    return out


# ------------------------------------------------------------------------------------------------ running the library
def _rows(lists, cap, B):
    a = np.full((B, cap), SENT32, np.int32)
    n = np.zeros(B, np.int32)
    for b, l in enumerate(lists):
        a[b, :len(l)] = l
        n[b] = len(l)
    return a, n


def _sentinel_out(B, cap_kf, cap_mp, backend):
    i32 = lambda *sh: to_dev_plain(np.full(sh, SENT32, np.int32), backend)   # noqa: E731
    u8 = lambda *sh: to_dev_plain(np.full(sh, SENT8, np.uint8), backend)     # noqa: E731
    return dict(local_kf=i32(B, cap_kf), n_local_kf=i32(B), n_local_kf_required=i32(B), ref_kf=i32(B), max_votes=i32(B),
                local_src=i32(B, cap_mp), nmp=i32(B), nmp_required=i32(B), local_mp=u8(B, cap_mp, 48), track=u8(B, cap_mp, 32), flags=i32(B))


def u8(a, itemsize):
    """the bytes of a record array from either backend, [..., itemsize]"""
    a = to_host(a)
    return a.view(np.uint8).reshape(a.shape + (itemsize,)) if a.dtype.names else a


def sync(backend):
    if backend == "hip":
        import torch
        torch.cuda.synchronize()


def run_and_check(lib, backend, W, frames, votes, flists=None, dropped=None, cap_kf=128, cap_mp=None, cap_f=None, expect_flags=None,
                  view=None):
    """votes / flists / dropped: per frame a list of map-point indices; flists None = the current frame votes (one aliased array).
    Runs the library, restates every frame and compares every output whole.  -> (the expected dicts, the library's dict, the view)"""
    B = len(votes)
    cap_mp = cap_mp or max(W.n_mp, 1)
    cap_f = cap_f or max([len(v) for v in votes] + [len(v) for v in (flists or [])] + [1]) + 3
    fr = np.zeros(B, LOCALMAP_FRAME_DTYPE)
    for b, (last_kf, fl) in enumerate(frames):
        fr[b] = (last_kf, fl)
    vote_a, n_vote = _rows(votes, cap_f, B)
    frame_a, n_frame = (vote_a, n_vote) if flists is None else _rows(flists, cap_f, B)
    m = orbhip.ORBmatcher(0.8, True, lib=lib)
    view = view or W.view(backend)
    d_vote = to_dev_plain(vote_a.copy(), backend)
    d_frame = d_vote if flists is None else to_dev_plain(frame_a.copy(), backend)
    dr = None
    if dropped is not None:
        drop_a, n_drop = _rows(dropped, max(max(len(d) for d in dropped), 1) + 2, B)
        dr = (to_dev_plain(drop_a, backend), to_dev_plain(n_drop, backend))
    out = m.UpdateLocalMap(view, to_dev(fr, backend), d_vote, to_dev_plain(n_vote, backend), d_frame, to_dev_plain(n_frame, backend),
                           cap_kf, cap_mp, dropped_mp=dr[0] if dr else None, n_dropped=dr[1] if dr else None,
                           out=_sentinel_out(B, cap_kf, cap_mp, backend))
    sync(backend)
    got = {k: to_host(v) for k, v in out.items() if k not in ("work", "cap_kf", "cap_mp")}
    trk_slab = u8(view["mp_track"], 32).reshape(-1, W.n_mp, 32).view(TRACK_DTYPE)[..., 0]
    exp = []
    for b in range(B):
        v = list(votes[b])
        f = v if flists is None else list(flists[b])
        e = ref_update_local_map(W, fr[b], v, f, dropped[b] if dropped else None, cap_kf, cap_mp, trk_slab[b if trk_slab.shape[0] > 1 else 0])
        exp.append(e)
        for name in ("n_local_kf", "n_local_kf_required", "ref_kf", "max_votes", "nmp", "nmp_required", "flags"):
            assert int(got[name][b]) == e[name], (b, name, int(got[name][b]), e[name])
        want_kf = np.full(cap_kf, SENT32, np.int32)
        want_kf[:e["n_local_kf"]] = e["local_kf"]
        assert np.array_equal(got["local_kf"][b], want_kf), (b, got["local_kf"][b][:12], want_kf[:12])
        want_src = np.full(cap_mp, SENT32, np.int32)
        want_src[:e["nmp"]] = e["local_src"]
        assert np.array_equal(got["local_src"][b], want_src), (b, got["local_src"][b][:12], want_src[:12])
        want_mp = np.full((cap_mp, 48), SENT8, np.uint8)
        want_trk = np.full((cap_mp, 32), SENT8, np.uint8)
        if e["nmp"]:
            want_mp[:e["nmp"]] = e["local_mp"].view(np.uint8).reshape(-1, 48)
            want_trk[:e["nmp"]] = e["track"].view(np.uint8).reshape(-1, 32)
        assert np.array_equal(got["local_mp"][b], want_mp), b
        assert np.array_equal(got["track"][b], want_trk), b
        # the lists: nulled in place, nothing past the count touched
        want_v = np.full(cap_f, SENT32, np.int32)
        want_v[:len(v)] = v
        assert np.array_equal(to_host(d_vote)[b], want_v), b
        want_f = np.full(cap_f, SENT32, np.int32)
        want_f[:len(f)] = f
        assert np.array_equal(to_host(d_frame)[b], want_f), b
        if expect_flags is not None:
            assert e["flags"] == expect_flags[b], (b, e["flags"])
    return exp, out, view


def frame_points(rng, W, n):
    """a frame's mvpMapPoints: n entries drawn from the map, a third of them empty"""
    v = rng.integers(0, W.n_mp, n)
    v[rng.random(n) < 0.3] = -1
    return [int(x) for x in v]


# ------------------------------------------------------------------------------------------------ list sizes, order, batches
@pytest.mark.parametrize("backend", BACKENDS)
def test_list_sizes_and_ragged_batch(lib, backend):
    """vote lists of 0 / 1 / 63 / 64 / 65 / 255 / 256 / 257 entries (cap_f no multiple of 64), kf_by_order a random permutation; then a ragged
    batch of five with separate lists and per-frame track slabs"""
    rng = np.random.default_rng(3)
    sizes = [0, 1, 63, 64, 65, 255, 256, 257]
    W8 = random_world(np.random.default_rng(4), 60, 900, 120, B=len(sizes))
    votes = [frame_points(rng, W8, n) for n in sizes]
    exp, _, _ = run_and_check(lib, backend, W8, [(-1, 0)] * len(sizes), votes, cap_f=263)
    assert exp[0]["n_local_kf_required"] == 0 and exp[0]["ref_kf"] == -1 and exp[0]["nmp"] == 0   # no votes: empty list, keep the reference
    assert exp[-1]["nmp"] > 100 and not np.array_equal(W8.order, np.arange(60))
    W5 = random_world(np.random.default_rng(5), 50, 700, 100, B=5)
    votes = [frame_points(rng, W5, n) for n in (200, 0, 37, 129, 256)]
    flists = [frame_points(rng, W5, n) for n in (10, 150, 0, 129, 258)]
    dropped = [frame_points(rng, W5, n) for n in (5, 0, 9, 1, 40)]
    exp, _, _ = run_and_check(lib, backend, W5, [(int(rng.integers(0, 50)), b & 1) for b in range(5)], votes, flists, dropped)
    assert sum(e["nmp"] for e in exp) > 300


# ------------------------------------------------------------------------------------------------ hand-made maps
def _kf(mp=(), **kw):
    d = dict(bad=False, parent=-1, prev=-1, mp=list(mp), covis=[], children=[])
    d.update(kw)
    return d


def hand_world(rng, kfs, n_mp, order=None, bad_mp=(), obs_extra=None, B=1):
    """observations = the key frames that hold the point, in pointer order (obs_extra[p] replaces a point's list)"""
    order = list(order) if order is not None else list(range(len(kfs)))
    rank = {k: r for r, k in enumerate(order)}
    obs = [[] for _ in range(n_mp)]
    for k in sorted(range(len(kfs)), key=lambda c: rank[c]):
        if kfs[k] is None:
            continue
        for p in dict.fromkeys(kfs[k]["mp"]):
            if 0 <= p < n_mp:
                obs[p].append((k, 0))
    for p, o in (obs_extra or {}).items():
        obs[p] = o
    fl = np.full(n_mp, MP_VALID | MP_HAS_OBS, np.uint32)
    for p in bad_mp:
        fl[p] |= MP_BAD
    return World(rng, kfs, fl, obs, order, B)


@pytest.mark.parametrize("backend", BACKENDS)
def test_pkfmax_ties_bad_and_empty(lib, backend):
    """ties in the maximum: the first in pointer order wins; a bad key frame with the most votes is neither listed nor pKFmax"""
    rng = np.random.default_rng(7)
    # key frames 0..3 hold points; pointer order 2, 0, 3, 1; 0 and 2 tie with 3 votes, 3 is bad with 4
    kfs = [_kf([0, 1, 2]), _kf([0]), _kf([1, 2, 3]), _kf([0, 1, 2, 3], bad=True)]
    W = hand_world(rng, kfs, 6, order=[2, 0, 3, 1])
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)], [[0, 1, 2, 3]], expect_flags=[0])
    assert exp[0]["ref_kf"] == 2 and exp[0]["max_votes"] == 3 and exp[0]["local_kf"] == [2, 0, 1]
    W = hand_world(rng, kfs, 6, order=[1, 0, 3, 2])
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)], [[0, 1, 2, 3]])
    assert exp[0]["ref_kf"] == 0 and exp[0]["local_kf"] == [1, 0, 2]
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)], [[4, 5, -1]])   # points nobody observes
    assert exp[0]["ref_kf"] == -1 and exp[0]["max_votes"] == 0 and exp[0]["n_local_kf"] == 0


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n1", [0, 1, 79, 80, 81, 120])
def test_first_level_sizes(lib, backend, n1):
    """the `size() > 80` break before, at and after the boundary; a first level above 80 is kept whole"""
    rng = np.random.default_rng(100 + n1)
    n_kf = 200
    kfs = []
    for k in range(n_kf):
        mp = [0] if k < n1 else []
        kfs.append(_kf(mp + [int(x) for x in rng.integers(1, 40, 6)], covis=[int(x) for x in rng.choice(n_kf, 10, replace=False)],
                       parent=int(rng.integers(0, n_kf)) if rng.random() < 0.02 else -1))
    W = hand_world(rng, kfs, 40, order=rng.permutation(n_kf), obs_extra={p: [] for p in range(1, 40)})
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)], [[0]], cap_kf=200)
    n = exp[0]["n_local_kf_required"]
    assert n >= n1 and (n == n1 if n1 > 80 or n1 == 0 else n > n1), (n1, n)
    if n1 in (79, 80):
        assert n <= 83   # the loop stops at the first iteration that sees more than 80


@pytest.mark.parametrize("backend", BACKENDS)
def test_first_level_and_segments_over_three_chunks(lib, backend):
    """600 ranks and 513 segments through the 256-lane chunk loops (csrc/wg_scan.inc): the third chunk writes the per-wave totals where the
    first did.  520 key frames in an irregular set hold the voted point, 7 of them bad, so the first level keeps 513 (no multiple of 64) of
    600 ranks; the key frames have 1 to 10 features, so the segment offsets are an irregular running sum"""
    rng = np.random.default_rng(513)
    n_kf, n_hold, n_bad = 600, 520, 7
    holders = rng.choice(n_kf, n_hold, replace=False)
    bad = set(int(k) for k in holders[:n_bad])
    hold = set(int(k) for k in holders)
    kfs = [_kf(([0] if k in hold else []) + [int(x) for x in rng.integers(1, 40, int(rng.integers(1, 10)))], bad=k in bad) for k in range(n_kf)]
    W = hand_world(rng, kfs, 40, order=rng.permutation(n_kf), obs_extra={p: [] for p in range(1, 40)})
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)], [[0]], cap_kf=n_kf, expect_flags=[0])
    assert exp[0]["n_local_kf"] == n_hold - n_bad == 513 and exp[0]["nmp"] == 40
    keep = np.array([int(k) in hold and int(k) not in bad for k in W.order])
    assert 0 < keep[:256].sum() < 256 and 0 < keep[256:512].sum() < 256 and 0 < keep[512:].sum() < 88   # every chunk keeps some, drops some


@pytest.mark.parametrize("backend", BACKENDS)
def test_second_loop(lib, backend):
    rng = np.random.default_rng(9)
    # 0: first level.  covis: 1 bad, 0 itself (listed), 2 usable but AFTER them, so 2 is taken; fewer than 10 covisibles.
    # children of 0: 1 (bad), 0 (listed), 3 -> the first usable one is the third.  parent of 0 = 4, bad: still added, and ends the loop.
    kfs = [_kf([0], covis=[1, 0, 2], children=[1, 0, 3], parent=4), _kf([], bad=True), _kf([]), _kf([]), _kf([], bad=True),
           _kf([0], covis=[6]), _kf([])]
    W = hand_world(rng, kfs, 2)
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)], [[0]], expect_flags=[0])
    # first level [0, 5]; from 0: covis 2, child 3, parent 4 -> break of the OUTER loop: 5 contributes nothing (6 is never added)
    assert exp[0]["local_kf"] == [0, 5, 2, 3, 4]
    # every covis entry bad or listed; the parent is already listed: no break, the next first-level key frame contributes
    kfs = [_kf([0], covis=[1, 5], parent=5), _kf([], bad=True), _kf([]), _kf([]), _kf([]), _kf([0], covis=[6], parent=3), _kf([]),
           _kf([0], covis=[2])]
    W = hand_world(rng, kfs, 2)
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)], [[0]], expect_flags=[0])
    assert exp[0]["local_kf"] == [0, 5, 7, 6, 3]   # 0 adds nothing; 5 adds covis 6 and parent 3, which ends the loop before 7


@pytest.mark.parametrize("backend", BACKENDS)
def test_inertial_tail(lib, backend):
    rng = np.random.default_rng(10)
    n_kf = 140
    kfs = [_kf([0] if k >= 100 and k < 100 + 2 else [], prev=k - 1 if k else -1) for k in range(n_kf)]
    W = hand_world(rng, kfs, 2, B=7)
    frames = [(5, LM_INERTIAL),     # a chain shorter than 20: 5, 4, .., 0
              (60, LM_INERTIAL),    # a chain of 25 available: 20 rounds
              (103, LM_INERTIAL),   # 103, 102, then 101 is listed: the chain stalls
              (-1, LM_INERTIAL), (60, 0), (300, LM_INERTIAL), (60, LM_INERTIAL)]
    exp, _, _ = run_and_check(lib, backend, W, frames, [[0]] * 7, cap_kf=130)
    assert exp[0]["local_kf"] == [100, 101, 5, 4, 3, 2, 1, 0]
    assert exp[1]["local_kf"] == [100, 101] + list(range(60, 40, -1))
    assert exp[2]["local_kf"] == [100, 101, 103, 102]
    assert exp[3]["local_kf"] == [100, 101] and exp[4]["local_kf"] == [100, 101]
    assert exp[5]["flags"] == LM_BAD_INDEX and exp[5]["local_kf"] == [100, 101]
    # size already >= 80: the tail does not run
    kfs = [_kf([0] if k < 80 else [], prev=k - 1 if k else -1) for k in range(n_kf)]
    W = hand_world(rng, kfs, 2)
    exp, _, _ = run_and_check(lib, backend, W, [(120, LM_INERTIAL)], [[0]], cap_kf=130)
    assert exp[0]["n_local_kf_required"] == 80
    kfs[79]["mp"] = []
    W = hand_world(rng, kfs, 2)
    exp, _, _ = run_and_check(lib, backend, W, [(120, LM_INERTIAL)], [[0]], cap_kf=130)
    assert exp[0]["n_local_kf_required"] == 99 and exp[0]["local_kf"][79] == 120


@pytest.mark.parametrize("backend", BACKENDS)
def test_observation_records(lib, backend):
    """a rig entry with left and right records counts once; two different key frames adjacent in the list both count; a RIGHT-only entry counts"""
    rng = np.random.default_rng(11)
    kfs = [_kf([0, 1, 2]), _kf([0, 1, 2]), _kf([0, 1, 2])]
    obs = {0: [(0, 0), (0, OBS_RIGHT), (1, 0)],            # kf 0 once, kf 1 once
           1: [(1, 0), (2, OBS_RIGHT)],                     # adjacent records of different key frames; 2 is RIGHT-only
           2: [(2, OBS_RIGHT), (2, OBS_RIGHT), (0, OBS_RIGHT), (7, 0), (0, 0)]}   # 2 once; 0 RIGHT-only; 7 out of range; 0 again (a new entry)
    W = hand_world(rng, kfs, 3, obs_extra=obs)
    exp, out, _ = run_and_check(lib, backend, W, [(-1, 0)], [[0, 1, 2]], expect_flags=[LM_BAD_INDEX])
    assert exp[0]["max_votes"] == 3 and exp[0]["ref_kf"] == 0   # 0: 1 + 0 + 2, 1: 1 + 1, 2: 0 + 1 + 1


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("aliased", [True, False])
def test_points(lib, backend, aliased):
    """the same point in several key frames and twice in one; bad points in key frames, in the frame list and in the vote list are nulled /
    never listed; points of the frame in no local key frame; a dropped list"""
    rng = np.random.default_rng(12)
    kfs = [_kf([0, 1, 1, 2, -1, 6]), _kf([2, 3, 0, 6, 4]), _kf([9])]
    W = hand_world(rng, kfs, 10, bad_mp=[6, 7])
    W.track["in_view"] = 1
    vote = [0, 7, 3, -1, 8, 6]          # 7 and 6 are bad; 8 is in no key frame
    flist = None if aliased else [1, 6, 8, 4, -1]
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)], [vote], None if aliased else [flist], dropped=[[2, 5, -1]], expect_flags=[0])
    e = exp[0]
    assert e["local_kf"] == [0, 1] and e["local_src"] == [2, 3, 0, 4, 1]   # reverse key-frame order, first occurrence wins
    seen = (e["local_mp"]["flags"] & MP_SEEN) != 0
    assert list(seen) == ([True, True, True, False, False] if aliased else [True, False, False, True, True])
    assert list(e["track"]["in_view"]) == [0, 1, 1, 1, 1]   # only the dropped point loses in_view; SEEN points keep the stale 1


@pytest.mark.parametrize("backend", BACKENDS)
def test_capacities(lib, backend):
    rng = np.random.default_rng(13)
    W = random_world(rng, 40, 500, 80, B=2)
    votes = [frame_points(rng, W, 150), frame_points(rng, W, 3)]
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)] * 2, votes)
    nk, nm = exp[0]["n_local_kf_required"], exp[0]["nmp_required"]
    assert nk > exp[1]["n_local_kf_required"] and nm > exp[1]["nmp_required"] > 0
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)] * 2, votes, cap_kf=nk - 1)
    assert exp[0]["flags"] & LM_KF_OVERFLOW and exp[0]["nmp"] == 0 and exp[0]["n_local_kf"] == nk - 1 and not exp[1]["flags"] & LM_KF_OVERFLOW
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)] * 2, votes, cap_mp=nm - 1)
    assert exp[0]["flags"] & LM_MP_OVERFLOW and exp[0]["nmp"] == nm - 1 and exp[0]["nmp_required"] == nm and exp[1]["nmp"] == exp[1]["nmp_required"]
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)] * 2, votes, cap_kf=nk, cap_mp=nm)
    assert not (exp[0]["flags"] | exp[1]["flags"]) & (LM_KF_OVERFLOW | LM_MP_OVERFLOW)


@pytest.mark.parametrize("backend", BACKENDS)
def test_bad_indices(lib, backend):
    """indices out of range everywhere they can occur, a slot that is not VALID, an absent key frame: skipped and flagged, nothing read out of
    bounds (the emulated build runs on exact-size host arrays)"""
    rng = np.random.default_rng(14)
    base = [_kf([0, 1, 2], covis=[1], children=[2], parent=3), _kf([3]), _kf([4]), _kf([5]), None, _kf([0])]

    def world(**change):
        kfs = [None if k is None else dict(k, mp=list(k["mp"]), covis=list(k["covis"]), children=list(k["children"])) for k in base]
        for key, val in change.items():
            kfs[0][key] = val
        return hand_world(rng, kfs, 8)

    clean, _, _ = run_and_check(lib, backend, world(), [(-1, 0)], [[0, 1]], expect_flags=[0])
    assert clean[0]["local_kf"] == [0, 5, 1, 2, 3]
    for change in (dict(mp=[0, 1, 99]), dict(mp=[0, -7, 2]), dict(covis=[17, 1]), dict(covis=[-2, 4, 1]), dict(children=[-1, 2]),
                   dict(children=[6, 4, 2]), dict(parent=4), dict(parent=44)):
        exp, _, _ = run_and_check(lib, backend, world(**change), [(-1, 0)], [[0, 1]], expect_flags=[LM_BAD_INDEX])
        assert exp[0]["local_kf"][:4] == [0, 5, 1, 2], change
    # list entries out of range, an invalid slot, in the vote list, the frame list and the dropped list
    W = world()
    W.mp["flags"][7] = 0
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)], [[0, 8, 1]], expect_flags=[LM_BAD_INDEX])
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)], [[0, 1]], [[0, -5, 7]], expect_flags=[LM_BAD_INDEX])
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)], [[0, 1]], [[0]], dropped=[[1, 1 << 30]], expect_flags=[LM_BAD_INDEX])
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)], [[7]], expect_flags=[LM_BAD_INDEX])
    assert exp[0]["n_local_kf"] == 0
    # rows past the table, a child range past the table, an observation of an absent key frame, a CSR range past the records
    W = world()
    W.kf[1]["n_feat"] = len(W.kf_mp)
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)], [[0, 1]], expect_flags=[LM_BAD_INDEX])
    assert exp[0]["local_kf"] == [0, 5, 1, 2, 3] and exp[0]["local_src"] == [5, 4, 0, 1, 2]
    W = world()
    W.kf[0]["mp_row0"] = -1
    run_and_check(lib, backend, W, [(-1, 0)], [[0, 1]], expect_flags=[LM_BAD_INDEX])
    W = world()
    W.kf[0]["n_child"] = len(W.children) + 1
    run_and_check(lib, backend, W, [(-1, 0)], [[0, 1]], expect_flags=[LM_BAD_INDEX])
    W = world()
    W.obs["kf"][W.obs_start[1]] = 4
    exp, _, _ = run_and_check(lib, backend, W, [(-1, 0)], [[1]], expect_flags=[LM_BAD_INDEX])
    assert exp[0]["n_local_kf"] == 0
    W = world()
    W.obs_start[2] = len(W.obs) + 5
    run_and_check(lib, backend, W, [(-1, 0)], [[0, 1, 2]], expect_flags=[LM_BAD_INDEX])


@pytest.mark.parametrize("backend", BACKENDS)
def test_realistic_size(lib, backend):
    """100 key frames x 1 000 features, about 6 000 distinct local points"""
    rng = np.random.default_rng(15)
    W = random_world(rng, 100, 6500, 1000, p_empty=0.4)
    W.kf_mp[W.kf_mp >= 0] = rng.integers(0, 6500, int((W.kf_mp >= 0).sum()))   # every key frame sees the whole map
    exp, _, _ = run_and_check(lib, backend, W, [(50, LM_INERTIAL)], [frame_points(rng, W, 1000)], cap_kf=128, cap_mp=6500)
    assert exp[0]["n_local_kf"] >= 80 and 5500 <= exp[0]["nmp"] <= 6500


def test_reversed_lane_order():
    """the emulated build under EMU_REVERSE=1 (lanes scheduled in reverse): the atomics make the result independent of the order"""
    env = dict(os.environ, EMU_REVERSE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", __file__, "-k",
                        "emu and (test_points or test_second_loop or test_capacities or test_list_sizes)"], env=env, cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ the chain with the projection
def _geometric_world(rng, n_mp, n_kf, n_feat):
    """a map whose records are a projectable scene (tests/test_map_projection.py make_scene) with key frames over it"""
    mp, _, desc, frames, track = tmp.make_scene(rng, PROJ_LOCAL_MAP, 1, n_mp, n_mp, special=False)
    W = random_world(rng, n_kf, n_mp, n_feat, p_bad_mp=0.0)
    fl = mp[0]["flags"] & ~np.uint32(MP_SEEN)
    fl[:] |= MP_VALID
    W.mp = mp[0].copy()
    W.mp["flags"] = fl
    W.track = track.copy()
    return W, desc, frames


def _host_path(m, backend, W, e, desc, frames, prm, cap_q):
    """the existing path: the restatement's host-built list, uploaded and projected"""
    n = e["nmp"]
    mp = np.zeros((1, max(n, 1)), MAP_POINT_DTYPE)
    trk = np.zeros((1, max(n, 1)), TRACK_DTYPE)
    mp[0, :n], trk[0, :n] = e["local_mp"], e["track"]
    d_trk = to_dev(trk, backend) if backend == "hip" else trk.copy()
    out = m.ProjectMapPoints(to_dev(mp, backend), to_dev_plain(np.array([n], np.int32), backend), to_dev_plain(desc, backend),
                             to_dev(frames, backend), prm, cap_q, track=d_trk)
    sync(backend)
    return out, u8(d_trk, 32).reshape(1, -1, 32)[0, :n]


@pytest.mark.parametrize("backend", BACKENDS)
def test_chain_with_projection(lib, backend):
    """update -> project(LOCAL_MAP) -> store -> a second frame: queries, q_src and tracks equal those of the existing path fed with the
    restatement's host-built list; a SEEN point whose stale in_view = 1 comes from the first frame produces a query in the second"""
    rng = np.random.default_rng(16)
    n_mp = 700
    W, desc, frames = _geometric_world(rng, n_mp, 30, 90)
    W.track["in_view"] = 0
    m = orbhip.ORBmatcher(0.8, True, lib=lib)
    prm = tmp.params(m, PROJ_LOCAL_MAP, 3.0)
    cap_q = n_mp
    view = W.view(backend)
    vote = frame_points(rng, W, 120)
    stale = None
    for it in range(2):
        slab_before = u8(view["mp_track"], 32).reshape(n_mp, 32).copy().view(TRACK_DTYPE)[:, 0]
        W.track = slab_before[None].copy()
        exp, loc, _ = run_and_check(lib, backend, W, [(-1, 0)], [vote], view=view)
        e = exp[0]
        assert e["nmp"] > 150
        proj = m.ProjectMapPoints(loc["local_mp"], loc["nmp"], to_dev_plain(desc, backend), to_dev(frames, backend), prm, cap_q,
                                  track=loc["track"])
        m.StoreLocalTracks(loc, view)
        sync(backend)
        ref, ref_trk = _host_path(m, backend, W, e, desc, frames, prm, cap_q)
        nq = int(to_host(ref["nq"])[0])
        assert nq > 20 and int(to_host(proj["nq"])[0]) == nq and int(to_host(proj["n_in_view"])[0]) == int(to_host(ref["n_in_view"])[0])
        for k in ("queries", "qdesc", "q_src"):
            assert np.array_equal(to_host(proj[k])[0, :nq], to_host(ref[k])[0, :nq]), (it, k)
        assert np.array_equal(to_host(loc["track"]).reshape(1, -1, 32)[0, :e["nmp"]], ref_trk), it
        # the scatter-back: the slab holds the projected entries of the local points, every other entry as before
        want = slab_before.copy().view(np.uint8).reshape(n_mp, 32)
        want[e["local_src"]] = ref_trk
        assert np.array_equal(u8(view["mp_track"], 32).reshape(n_mp, 32), want), it
        if it == 0:
            q_src = to_host(proj["q_src"])[0, :nq]
            stale = int(e["local_src"][q_src[0]])   # in view in frame 1: in_view = 1 is in the slab now
            vote = [stale] + frame_points(rng, W, 60)   # frame 2 matched it: SEEN, isInFrustum skipped
        else:
            j = e["local_src"].index(stale)
            assert e["local_mp"]["flags"][j] & MP_SEEN and e["track"]["in_view"][j] == 1
            assert j in to_host(proj["q_src"])[0, :nq]   # the quirk: the stale mbTrackInView still produces a query


@pytest.mark.gpu
def test_graph_capture_replay_hip(hip_lib):
    """update -> project -> store captured on one stream, replayed twice on changed frame lists == the eager calls"""
    import torch
    rng = np.random.default_rng(17)
    n_mp, B, cap_f, cap_kf = 700, 3, 150, 64
    W, desc, frames = _geometric_world(rng, n_mp, 30, 90)
    W.track = np.repeat(W.track, B, 0)
    m = orbhip.ORBmatcher(0.8, True, lib=hip_lib)
    prm = tmp.params(m, PROJ_LOCAL_MAP, 3.0)
    view = W.view("hip")
    track0 = view["mp_track"].clone()
    fr = np.zeros(B, LOCALMAP_FRAME_DTYPE)
    fr["last_kf"] = -1
    d_fr, d_desc, d_pf = to_dev(fr, "hip"), to_dev_plain(desc, "hip"), to_dev(np.repeat(frames, B), "hip")
    lists = [_rows([frame_points(rng, W, n) for n in ns], cap_f, B) for ns in ((100, 0, 140), (30, 150, 77))]
    d_vote, d_n = to_dev_plain(lists[0][0], "hip"), to_dev_plain(lists[0][1], "hip")

    def step(loc=None, proj=None):
        loc = m.UpdateLocalMap(view, d_fr, d_vote, d_n, d_vote, d_n, cap_kf, n_mp, out=loc)
        proj = m.ProjectMapPoints(loc["local_mp"], loc["nmp"], d_desc, d_pf, prm, n_mp, track=loc["track"], out=proj)
        m.StoreLocalTracks(loc, view)
        return loc, proj

    def snapshot(loc, proj):
        torch.cuda.synchronize()
        nmp, nq = loc["nmp"].cpu().numpy(), proj["nq"].cpu().numpy()
        return ([loc[k].cpu().numpy() for k in ("n_local_kf_required", "ref_kf", "nmp_required", "flags")] + [nmp, nq] +
                [np.concatenate([loc[k].cpu().numpy()[b, :nmp[b]].reshape(-1) for b in range(B)]) for k in ("local_src", "local_mp", "track")] +
                [np.concatenate([proj[k].cpu().numpy()[b, :nq[b]].reshape(-1) for b in range(B)]) for k in ("queries", "q_src")] +
                [view["mp_track"].cpu().numpy(), d_vote.cpu().numpy()])

    eager = []
    for a, n in lists:   # two frames in a row: the second reads the tracks the first stored
        d_vote.copy_(torch.from_numpy(a))
        d_n.copy_(torch.from_numpy(n))
        eager.append(snapshot(*step()))
    assert eager[0][4].sum() > 200 and eager[1][5].sum() > 20
    view["mp_track"].copy_(track0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        loc, proj = step()   # allocates the outputs and the workspace outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(loc, proj)
    view["mp_track"].copy_(track0)
    for r, ((a, n), want) in enumerate(zip(lists, eager)):
        d_vote.copy_(torch.from_numpy(a))
        d_n.copy_(torch.from_numpy(n))
        torch.cuda.synchronize()
        g.replay()
        got = snapshot(loc, proj)
        for i, (x, y) in enumerate(zip(got, want)):
            assert np.array_equal(x, y), (r, i, x[:8], y[:8])


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("backend", BACKENDS)
def test_argument_errors(lib, backend):
    rng = np.random.default_rng(18)
    W = random_world(rng, 6, 40, 10)
    v = W.view(backend)
    m = orbhip.ORBmatcher(0.8, True, lib=lib)
    V = m._local_map_view(v)
    B = 1
    keep = [to_dev_plain(np.full((2, 8), -1, np.int32), backend), to_dev_plain(np.zeros(2, np.int32), backend), to_dev(np.zeros(2, LOCALMAP_FRAME_DTYPE), backend)]
    o = _sentinel_out(2, 4, 16, backend)
    work = m.LocalMapWorkspace(v, 2)
    a = lambda x: orbhip.matcher._addr(x)   # noqa: E731
    lists = lambda: LocalMapLists(a(keep[0]), a(keep[1]), a(keep[0]), a(keep[1]), None, None, 8, 0)   # noqa: E731
    outs = lambda: LocalMapOut(*[a(o[k]) for k in ("local_kf", "n_local_kf", "n_local_kf_required", "ref_kf", "max_votes", "local_src", "nmp",  # noqa: E731
                                                   "nmp_required", "local_mp", "track", "flags")], 4, 16)
    view = lambda: LocalMapView.from_buffer_copy(V)   # noqa: E731

    def call(Vv=None, L=None, O=None, batch=B, frames=keep[2], wk=work):
        Vv, L, O = Vv or view(), L or lists(), O or outs()
        return lib.orbm_update_local_map(C.byref(Vv), orbhip.matcher.ptr(frames), C.byref(L), batch, C.byref(O), orbhip.matcher.ptr(wk), None)

    assert call() == 0 and call(batch=0) == 0
    sync(backend)
    assert call(batch=-1) == ORB_E_INVALID and call(frames=None) == ORB_E_INVALID and call(wk=None) == ORB_E_INVALID
    assert lib.orbm_update_local_map(None, None, None, 1, None, None, None) == ORB_E_INVALID
    for name, _ in LocalMapView._fields_[:8]:
        x = view()
        setattr(x, name, None)
        assert call(Vv=x) == ORB_E_INVALID, name
    for name in ("n_mp", "n_obs", "n_kf", "n_kf_mp_rows", "n_children", "track_stride"):
        x = view()
        setattr(x, name, -1)
        assert call(Vv=x) == ORB_E_INVALID, name
    assert call(batch=2) == ORB_E_INVALID   # track_stride 0 with batch > 1
    x = view()
    x.track_stride = W.n_mp - 1
    assert call(Vv=x) == ORB_E_INVALID
    x = view()
    x.d_mp_track = x.d_mp_track + 4
    assert call(Vv=x) == ORB_E_INVALID      # misaligned slab
    for name in ("d_vote_mp", "d_n_vote", "d_frame_mp", "d_n_frame"):
        x = lists()
        setattr(x, name, None)
        assert call(L=x) == ORB_E_INVALID, name
    x = lists()
    x.cap_f = 0
    assert call(L=x) == ORB_E_INVALID
    x = lists()
    x.d_dropped_mp = x.d_vote_mp
    assert call(L=x) == ORB_E_INVALID       # a dropped list without its counts / capacity
    for name, _ in LocalMapOut._fields_[:11]:
        x = outs()
        setattr(x, name, None)
        assert call(O=x) == ORB_E_INVALID, name
    for name in ("cap_kf", "cap_mp"):
        x = outs()
        setattr(x, name, 0)
        assert call(O=x) == ORB_E_INVALID, name
    # orbm_store_local_tracks
    p = orbhip.matcher.ptr
    store = lambda t=o["track"], s=o["local_src"], n=o["nmp"], cap=16, b=1, slab=v["mp_track"], stride=0, nmp=W.n_mp: \
        lib.orbm_store_local_tracks(p(t), p(s), p(n), cap, b, p(slab), stride, nmp, None)   # noqa: E731
    assert store(n=keep[1]) == 0 and store(b=0) == 0
    sync(backend)
    assert [store(t=None), store(s=None), store(n=None), store(slab=None), store(cap=0), store(b=-1), store(b=2), store(stride=3),
            store(nmp=-1)] == [ORB_E_INVALID] * 9
    assert lib.orbm_local_map_workspace_bytes(-1, 1, 1) == 0 and lib.orbm_local_map_workspace_bytes(10, 100, 2) >= 2 * 4 * (3 * 10 + 100)
    with pytest.raises(orbhip.OrbHipError):
        m.check_local_map(dict(flags=np.array([LM_BAD_INDEX]), n_local_kf_required=np.array([1]), nmp_required=np.array([1]), cap_kf=4, cap_mp=4))
    with pytest.raises(orbhip.OrbHipError):
        m.check_local_map(dict(flags=np.array([0]), n_local_kf_required=np.array([5]), nmp_required=np.array([1]), cap_kf=4, cap_mp=4))
    assert QUERY_DTYPE.itemsize == 28
