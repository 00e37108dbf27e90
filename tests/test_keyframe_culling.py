"""LocalMapping::KeyFrameCulling on the device map (include/orbhip.h "Key-frame culling"): orbm_cull_keyframes and orbm_apply_keyframe_culling
against a literal Python restatement of LocalMapping.cc:1176-1321, KeyFrame::SetBadFlag's early returns and EraseObservation loop
(KeyFrame.cc:651-688), MapPoint::EraseObservation (MapPoint.cc:197-231) and MapPoint::SetBadFlag (:254-277), written over dicts and lists as
the reference holds them.  Integer work and decisions: every output is compared bit for bit, the bytes past the counts against a sentinel.
Every constructed case is also run through a deliberately wrong variant OF THE RESTATEMENT, so that the case is known to discriminate."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import orbhip
from devarrays import BACKENDS, lib, to_dev, to_dev_plain, to_host  # noqa: F401
from orbhip._abi import (CULL_ABORT_BA, CULL_BAD_INDEX, CULL_CODE_CULLED, CULL_CODE_CULLED_IMU1, CULL_CODE_CULLED_IMU2, CULL_CODE_DEFERRED,
                         CULL_CODE_KEPT, CULL_CODE_KEPT_FEW_KFS, CULL_CODE_KEPT_INERTIAL, CULL_CODE_KEPT_NO_NEIGHBOUR, CULL_CODE_KEPT_RECENT,
                         CULL_CODE_NOT_VISITED, CULL_CODE_SKIPPED, CULL_IMU_INITIALIZED, CULL_INERTIAL, CULL_INERTIAL_BA2,
                         CULL_MONOCULAR, CULL_PROBLEM_DTYPE, CULL_REC_ERASED_BY_KF, CULL_REC_ERASED_BY_POINT, CULL_REC_LIVE,
                         CULL_UNSUPPORTED, LM_KF_BAD, MAP_POINT_DTYPE, MP_BAD, MP_HAS_OBS, MP_VALID, OBS_RIGHT, ORB_E_INVALID,
                         REFRESH_POINT_DTYPE, CullApply, CullIn, CullOut, CullWorkspaceLayout)
from orbhip.matcher import flatten_cull_keyframes, flatten_local_map_keyframes, flatten_observations

SENT8 = 0x5A
SENT32 = 0x5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WG = 1024   # the lanes of k_cull_walk's workgroup (csrc/orbm_culling.hip CULL_WG)


# ------------------------------------------------------------------------------------------------ a map as the reference holds it
def KF(mp=(), octave=None, close=None, stereo=None, **kw):
    """one key frame: mp = mvpMapPoints as point indices (None = NULL)"""
    n = len(mp)
    d = dict(id=None, bad=False, mp=list(mp), octave=list(octave) if octave is not None else [0] * n,
             close=list(close) if close is not None else [True] * n, stereo=list(stereo) if stereo is not None else [False] * n,
             prev=None, next=None, ts=0.0, pos=(0.0, 0.0, 0.0), not_erase=False, to_be_erased=False)
    d.update(kw)
    return d


class Map:
    """kfs: list of KF dicts (or None for an empty slot); mps: list of dict(bad, nObs, obs = {kf: leftIndex} in mObservations' iteration order,
    ref = mpRefKF).  Observations are derived from the key frames (the FIRST feature that holds a point is the entry's leftIndex) in key-frame
    index order unless `order` gives the pointer order."""

    def __init__(self, kfs, n_mp, order=None, bad_mp=(), nobs=None, no_obs=()):
        self.kfs = kfs
        for i, k in enumerate(kfs):
            if k is not None and k["id"] is None:
                k["id"] = i
        self.mps = [dict(bad=p in bad_mp, nObs=0, obs={}, ref=None) for p in range(n_mp)]
        for k in (order if order is not None else range(len(kfs))):
            if kfs[k] is None:
                continue
            for i, p in enumerate(kfs[k]["mp"]):
                if p is None or not 0 <= p < n_mp or (k, p) in no_obs or k in self.mps[p]["obs"]:
                    continue
                self.mps[p]["obs"][k] = i
                self.mps[p]["nObs"] += 2 if kfs[k]["stereo"][i] else 1   # AddObservation (MapPoint.cc:191-194)
        for p, m in enumerate(self.mps):
            m["ref"] = next(iter(m["obs"]), 0)
            if nobs and p in nobs:
                m["nObs"] = nobs[p]
            if m["bad"]:   # MapPoint::SetBadFlag already ran (nObs: what the records give, as with d_mp_nobs == NULL)
                for k, i in m["obs"].items():
                    kfs[k]["mp"][i] = None
                m["obs"] = {}
                m["nObs"] = nobs[p] if nobs and p in nobs else 0
        self.fate = {}   # (point, kf) -> CULL_REC_ERASED_BY_KF / _BY_POINT


def problem(cur, cands, init_id=0xFFFFFFF0, n_in_map=None, inertial=False, mono=False, imu_init=False, ba2=False, abort=False):
    return dict(cur=cur, cands=list(cands), init_id=init_id, n_in_map=n_in_map, inertial=inertial, mono=mono, imu_init=imu_init, ba2=ba2,
                abort=abort)


# ------------------------------------------------------------------------------------------------ the reference, restated
def ref_keyframe_culling(M, P, variant=None):
    """LocalMapping::KeyFrameCulling on M (changed in place).  variant: one deliberate mistake.  -> dict(code, nmps, nred, events, n_in_map)"""
    kfs, mps = M.kfs, M.mps
    n_in_map = [P["n_in_map"] if P["n_in_map"] is not None else sum(k is not None and not k["bad"] for k in kfs)]
    n_static = n_in_map[0]

    def mp_set_bad(p):   # MapPoint::SetBadFlag
        m = mps[p]
        m["bad"] = True
        obs, m["obs"] = m["obs"], {}
        for k, left in obs.items():
            M.fate[(p, k)] = CULL_REC_ERASED_BY_POINT
            kfs[k]["mp"][left] = None   # EraseMapPointMatch(leftIndex)

    def erase_observation(p, k):   # MapPoint::EraseObservation
        m = mps[p]
        if k in m["obs"]:
            left = m["obs"][k]
            m["nObs"] -= 2 if (kfs[k]["stereo"][left] and variant != "weight_one") else 1
            del m["obs"][k]
            M.fate[(p, k)] = CULL_REC_ERASED_BY_KF
            if m["ref"] == k and m["obs"]:
                m["ref"] = next(iter(m["obs"]))
            if m["nObs"] <= 2 and variant != "never_bad":
                mp_set_bad(p)
        elif variant == "dup_twice":
            m["nObs"] -= 1

    def kf_set_bad(k):   # KeyFrame::SetBadFlag -> deferred?
        K = kfs[k]
        if K["id"] == P["init_id"]:
            return False
        if K["not_erase"]:
            K["to_be_erased"] = True
            return True
        for p in list(K["mp"]):
            if p is not None:
                erase_observation(p, k)
        K["bad"] = True
        n_in_map[0] -= 1
        return False

    Nd = 21
    inertial, mono = P["inertial"], P["mono"]
    redundant_th = np.float32(0.9) if (not inertial or mono) else np.float32(0.5)
    cur = kfs[P["cur"]]
    last_ID = None
    if inertial:
        count, aux = 0, P["cur"]
        while count < Nd and kfs[aux]["prev"] is not None:
            aux = kfs[aux]["prev"]
            count += 1
        last_ID = kfs[aux]["id"]
    links0 = {i: (k["prev"], k["next"]) for i, k in enumerate(kfs) if k is not None}
    snapshot = copy.deepcopy(mps) if variant == "parallel" else None
    n = len(P["cands"])
    code, nmps, nred, events = [CULL_CODE_NOT_VISITED] * n, [0] * n, [0] * n, []
    count = 0
    for c, k in enumerate(P["cands"]):
        count += 1
        K = kfs[k]
        stop = (count > 20 and P["abort"]) or count > 100
        if variant == "break_top" and stop:
            break
        if K["id"] == P["init_id"] or K["bad"]:
            code[c] = CULL_CODE_SKIPPED
            continue
        src = snapshot if snapshot is not None else mps
        nRed = nMPs = 0
        for i, p in enumerate(K["mp"]):
            if p is None:
                continue
            m = src[p]
            if m["bad"]:
                continue
            if (not mono or variant == "close_always") and variant != "close_never" and not K["close"][i]:
                continue
            nMPs += 1
            if m["nObs"] > 3:
                scaleLevel = K["octave"][i]
                nObs = 0
                for ki, left in m["obs"].items():
                    if ki == k:
                        continue
                    if kfs[ki]["octave"][left] <= scaleLevel + {"octave_two": 2, "octave_zero": 0}.get(variant, 1):
                        nObs += 1
                        if nObs > 3:
                            break
                if nObs > (2 if variant == "three_enough" else 3):
                    nRed += 1
        nmps[c], nred[c] = nMPs, nRed
        if variant == "double_th":
            redundant = nRed > float(redundant_th) * nMPs
        else:
            redundant = bool(np.float32(nRed) > redundant_th * np.float32(nMPs))
        code[c] = CULL_CODE_KEPT
        if redundant:
            if inertial:
                if (n_static if variant == "static_count" else n_in_map[0]) <= Nd:
                    code[c] = CULL_CODE_KEPT_FEW_KFS
                    continue
                if variant == "signed_id":
                    recent = K["id"] > cur["id"] - 2
                else:
                    recent = K["id"] > ((cur["id"] - 2) & 0xFFFFFFFF)
                if recent:
                    code[c] = CULL_CODE_KEPT_RECENT
                    continue
                if K["prev"] is not None and K["next"] is not None:
                    pv, nx = (links0[k] if variant == "static_links" else (K["prev"], K["next"]))
                    t = np.float32(np.float64(kfs[nx]["ts"]) - np.float64(kfs[pv]["ts"]))
                    d = np.asarray(K["pos"], np.float32) - np.asarray(kfs[K["prev"]]["pos"], np.float32)   # float Mat subtraction
                    norm = np.sqrt(np.float64(0) + np.float64(d[0]) * np.float64(d[0]) + np.float64(d[1]) * np.float64(d[1]) +
                                   np.float64(d[2]) * np.float64(d[2]))
                    near = (np.float32(norm) < np.float32(0.02)) if variant == "float_norm" else (norm < 0.02)
                    first = (P["imu_init"] and K["id"] < last_ID and t < 3.) or (t < 0.5)
                    if first or (not P["ba2"] and near and t < 3):
                        pv, nx = K["prev"], K["next"]
                        kfs[nx]["prev"] = pv
                        kfs[pv]["next"] = nx
                        K["next"] = None
                        K["prev"] = None
                        events.append((k, pv, nx))
                        deferred = kf_set_bad(k)
                        code[c] = (CULL_CODE_CULLED_IMU1 if first else CULL_CODE_CULLED_IMU2) | (CULL_CODE_DEFERRED if deferred else 0)
                    else:
                        code[c] = CULL_CODE_KEPT_INERTIAL
                else:
                    code[c] = CULL_CODE_KEPT_NO_NEIGHBOUR
            else:
                events.append((k, -1, -1))
                code[c] = CULL_CODE_CULLED | (CULL_CODE_DEFERRED if kf_set_bad(k) else 0)
        if variant != "break_top" and stop:
            break
    return dict(code=code, nmps=nmps, nred=nred, events=events, n_in_map=n_in_map[0],
                final=([m["nObs"] for m in mps], [m["bad"] for m in mps]))


# ------------------------------------------------------------------------------------------------ flattening and running
def flatten(M, pass_nobs=True):
    """the device map of M: (view arrays, cull arrays, ref, desc_row0 per key frame, the (point, kf) of every record)"""
    recs = [None if k is None else dict(bad=k["bad"], mp=[-1 if p is None else p for p in k["mp"]],
                                        prev=-1 if k["prev"] is None else k["prev"], next=-1 if k["next"] is None else k["next"],
                                        id=k["id"], timestamp=k["ts"], imu_pos=k["pos"], not_erase=k["not_erase"], octave=k["octave"])
            for k in M.kfs]
    kf, kf_mp, _ = flatten_local_map_keyframes(recs)
    ckf, feat = flatten_cull_keyframes(recs)
    for i, k in enumerate(M.kfs):   # CLOSE / STEREO as given (flatten_cull_keyframes' depth / u_right path has its own test)
        if k is not None:
            r0 = int(kf[i]["mp_row0"])
            feat[r0:r0 + len(k["mp"])] = [o | (0x40 if c else 0) | (0x80 if s else 0) for o, c, s in zip(k["octave"], k["close"], k["stereo"])]
    row0 = ckf["desc_row0"].copy()
    obs_start, obs = flatten_observations([[(k, int(row0[k]) + left, 0) for k, left in m["obs"].items()] for m in M.mps])
    owner = [(p, k) for p, m in enumerate(M.mps) for k in m["obs"]]
    mp = np.zeros(len(M.mps), MAP_POINT_DTYPE)
    mp["flags"] = [MP_VALID | (MP_BAD if m["bad"] else 0) | (MP_HAS_OBS if m["nObs"] > 0 else 0) for m in M.mps]
    ref = np.zeros(len(M.mps), REFRESH_POINT_DTYPE)
    ref["ref_kf"], ref["level"] = [m["ref"] for m in M.mps], 7
    nobs = np.asarray([m["nObs"] for m in M.mps], np.int32)
    return dict(mp=mp, obs_start=obs_start, obs=obs, kf=kf, kf_mp=kf_mp), dict(ckf=ckf, feat=feat, mp_nobs=nobs if pass_nobs else None), ref, owner


def problems_array(M, probs):
    pr = np.zeros(len(probs), CULL_PROBLEM_DTYPE)
    cands = []
    for b, P in enumerate(probs):
        n_in = P["n_in_map"] if P["n_in_map"] is not None else sum(k is not None and not k["bad"] for k in M.kfs)
        fl = (CULL_INERTIAL if P["inertial"] else 0) | (CULL_MONOCULAR if P["mono"] else 0) | (CULL_IMU_INITIALIZED if P["imu_init"] else 0) | \
            (CULL_INERTIAL_BA2 if P["ba2"] else 0) | (CULL_ABORT_BA if P["abort"] else 0)
        pr[b] = (P["cur"], P["init_id"], len(cands), len(P["cands"]), n_in, fl)
        cands += P["cands"]
    return pr, np.asarray(cands + [SENT32], np.int32)[:len(cands)].copy() if cands else np.zeros(0, np.int32)


def rec_dev(a, backend):
    """to_dev of a copy; an empty record array keeps its count of 0 (its pointer may be null)"""
    if backend == "hip" and a.size == 0:
        import torch
        return torch.zeros((0, a.dtype.itemsize), dtype=torch.uint8, device="cuda")
    return to_dev(a.copy(), backend)


def dev_view(view, cull, backend):
    rec = lambda a: rec_dev(a, backend)   # noqa: E731
    dv = dict(mp=rec(view["mp"]), obs_start=to_dev_plain(view["obs_start"].copy(), backend), obs=rec(view["obs"]), kf=rec(view["kf"]),
              kf_mp=to_dev_plain(view["kf_mp"].copy(), backend))
    dc = dict(ckf=rec(cull["ckf"]), feat=to_dev_plain(cull["feat"].copy(), backend),
              mp_nobs=None if cull["mp_nobs"] is None else to_dev_plain(cull["mp_nobs"].copy(), backend))
    return dv, dc


def sentinel_out(B, cap, backend):
    return dict(code=to_dev_plain(np.full((B, cap), SENT8, np.uint8), backend), nmps=to_dev_plain(np.full((B, cap), SENT32, np.int32), backend),
                nred=to_dev_plain(np.full((B, cap), SENT32, np.int32), backend),
                events=to_dev_plain(np.full((B, cap, 12), SENT8, np.uint8), backend),
                n_events=to_dev_plain(np.full(B, SENT32, np.int32), backend), flags=to_dev_plain(np.full(B, SENT32, np.int32), backend))


def sync(backend):
    if backend == "hip":
        import torch
        torch.cuda.synchronize()


def u8(a):
    a = to_host(a)
    return a.view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else a


def expected_state(M0, M, owner):
    """the workspace sections the restatement's final map M implies (M0: the map before)"""
    rec = np.asarray([CULL_REC_LIVE if k in M.mps[p]["obs"] else M.fate[(p, k)] for p, k in owner], np.uint8).reshape(-1)
    link = lambda v: -1 if v is None else v   # noqa: E731
    return dict(nobs=np.asarray([m["nObs"] for m in M.mps], np.int32).reshape(-1), rec=rec,
                mp_bad=np.asarray([m["bad"] for m in M.mps], np.uint8).reshape(-1),
                kf_erased=np.asarray([k is not None and k["bad"] and not M0.kfs[i]["bad"] for i, k in enumerate(M.kfs)], np.uint8).reshape(-1),
                prev=np.asarray([-1 if k is None else link(k["prev"]) for k in M.kfs], np.int32).reshape(-1),
                next=np.asarray([-1 if k is None else link(k["next"]) for k in M.kfs], np.int32).reshape(-1))


def run_and_check(lib, backend, M0, probs, cap_cand=None, corrupt=None, expect_flags=0, absent=None, pass_nobs=True, apply=None, cap_obs_out=None,
                  variants=()):
    """Runs the library on the flattened M0 for all problems and compares every output with the restatement run on a copy of M0 (of
    absent(M0) where `corrupt` damages the flattened arrays).  apply: the problem to fold into the map, compared slab by slab.
    variants: wrong variants of the restatement that must give another outcome for problem 0.  -> (expected dicts, the final maps)"""
    B = len(probs)
    view, cull, ref, owner = flatten(M0, pass_nobs)
    pr, cands = problems_array(M0, probs)
    if corrupt:
        corrupt(view, cull, pr, cands)
    cap_cand = cap_cand or max(max(len(P["cands"]) for P in probs), 1) + 2
    m = orbhip.ORBmatcher(0.8, True, lib=lib)
    dv, dc = dev_view(view, cull, backend)
    out = m.CullKeyFrames(dv, dc, to_dev(pr, backend), to_dev_plain(cands, backend), cap_cand, n_cand_max=max(len(P["cands"]) for P in probs),
                          out=sentinel_out(B, cap_cand, backend))
    sync(backend)
    exp, finals = [], []
    for b, P in enumerate(probs):
        M = copy.deepcopy(absent(M0) if absent else M0)
        e = ref_keyframe_culling(M, P)
        exp.append(e)
        finals.append(M)
        n = len(P["cands"])
        want = np.full(cap_cand, SENT8, np.uint8)
        want[:n] = e["code"]
        assert np.array_equal(to_host(out["code"])[b], want), (b, to_host(out["code"])[b][:n], e["code"])
        for name in ("nmps", "nred"):
            want = np.full(cap_cand, SENT32, np.int32)
            want[:n] = e[name]
            assert np.array_equal(to_host(out[name])[b], want), (b, name, to_host(out[name])[b][:n], e[name])
        assert int(to_host(out["n_events"])[b]) == len(e["events"]), (b, e["events"])
        want = np.full((cap_cand, 12), SENT8, np.uint8)
        if e["events"]:
            want[:len(e["events"])] = np.asarray(e["events"], np.int32).view(np.uint8).reshape(-1, 12)
        assert np.array_equal(to_host(out["events"])[b], want), (b, e["events"])
        assert int(to_host(out["flags"])[b]) == expect_flags, (b, int(to_host(out["flags"])[b]))
        if not corrupt:
            st, want_st = m.CullState(dv, out, b), expected_state(M0, M, owner)
            for name in want_st:
                assert np.array_equal(st[name], want_st[name]), (b, name, st[name], want_st[name])
    for v in variants:
        w = ref_keyframe_culling(copy.deepcopy(M0), probs[0], variant=v)
        assert any(w[key] != exp[0][key] for key in ("code", "nmps", "nred", "events", "final")), v
    if expect_flags:
        with pytest.raises(orbhip.OrbHipError):
            m.check_cull_flags(out)
    else:
        m.check_cull_flags(out)
    if apply is not None:
        check_apply(m, backend, M0, finals[apply], view, cull, ref, owner, dv, dc, out, apply, cap_obs_out)
    return exp, finals


def check_apply(m, backend, M0, M, view, cull, ref, owner, dv, dc, out, b, cap_obs_out=None):
    """ApplyKeyFrameCulling of problem b against the restatement's final map M, every slab whole"""
    n_mp, n_live = len(M.mps), sum(len(x["obs"]) for x in M.mps)
    cap = n_live + 3 if cap_obs_out is None else cap_obs_out
    d_ref = to_dev(ref.copy(), backend)
    before = {k: u8(v).copy() for k, v in list(dv.items()) + [("ckf", dc["ckf"]), ("ref", d_ref)]}
    app = dict(obs_start=to_dev_plain(np.full(n_mp + 1, SENT32, np.int32), backend),
               obs=to_dev_plain(np.full((max(cap, 1), 12), SENT8, np.uint8), backend), result=to_dev_plain(np.full(2, SENT32, np.int32), backend))
    m.ApplyKeyFrameCulling(dv, dc, out, d_ref, cap, problem=b, out=app)
    sync(backend)
    res = to_host(app["result"])
    assert list(res) == [n_live, 1 if n_live > cap else 0]
    if n_live > cap:   # nothing is written, and the host check says so
        for k in before:
            assert np.array_equal(u8(dv[k] if k in dv else (dc["ckf"] if k == "ckf" else d_ref)), before[k]), k
        assert np.all(to_host(app["obs_start"]) == SENT32) and np.all(to_host(app["obs"]) == SENT8)
        with pytest.raises(orbhip.OrbHipError):
            m.check_cull_applied(app)
        return
    m.check_cull_applied(app)
    row0 = cull["ckf"]["desc_row0"]
    want_start, want_obs = flatten_observations([[(k, int(row0[k]) + left, 0) for k, left in x["obs"].items()] for x in M.mps])
    assert np.array_equal(to_host(app["obs_start"]), want_start)
    got_obs = to_host(app["obs"])
    assert np.array_equal(got_obs[:n_live], u8(want_obs).reshape(-1, 12)) and np.all(got_obs[n_live:] == SENT8)   # CSR order kept
    mp = view["mp"].copy()
    mp["flags"] = [MP_VALID | (MP_BAD if x["bad"] else 0) | (MP_HAS_OBS if x["nObs"] > 0 else 0) for x in M.mps]
    assert np.array_equal(u8(dv["mp"]), u8(mp))
    if dc["mp_nobs"] is not None:
        assert np.array_equal(to_host(dc["mp_nobs"]), [x["nObs"] for x in M.mps])
    kf = view["kf"].copy()
    ckf = cull["ckf"].copy()
    for i, k in enumerate(M.kfs):
        if k is None:
            continue
        kf[i]["flags"] |= LM_KF_BAD if k["bad"] else 0
        kf[i]["prev"] = ckf[i]["prev"] = -1 if k["prev"] is None else k["prev"]
        ckf[i]["next"] = -1 if k["next"] is None else k["next"]
    assert np.array_equal(u8(dv["kf"]), u8(kf)) and np.array_equal(u8(dc["ckf"]), u8(ckf))
    rows = [-1 if p is None else p for k in M.kfs if k is not None for p in k["mp"]]   # EraseMapPointMatch left NULLs; an erased key frame keeps its row
    assert np.array_equal(to_host(dv["kf_mp"]), np.asarray(rows, np.int32).reshape(-1))
    want_ref = ref.copy()
    for p, x in enumerate(M.mps):
        if not x["bad"] and x["ref"] != M0.mps[p]["ref"]:
            left = x["obs"][x["ref"]]
            want_ref[p] = (x["ref"], M.kfs[x["ref"]]["octave"][left])   # mObservations.begin()->first, and that feature's octave
    assert np.array_equal(u8(d_ref), u8(want_ref))
    assert np.array_equal(u8(dv["obs"]), before["obs"]) and np.array_equal(to_host(dv["obs_start"]), view["obs_start"])   # inputs untouched


def codes(e):
    return list(e["code"])


# ------------------------------------------------------------------------------------------------ the constructed cases
def shared_world(n_kf, n_feat, n_extra=4, octave=0, **kw):
    """n_kf key frames that all hold the same n_feat points, plus n_extra observers at the end that are never candidates"""
    return Map([KF(range(n_feat), octave=[octave] * n_feat, **kw) for _ in range(n_kf + n_extra)], n_feat)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("nf", [3, 64, 65, 70])
def test_chain_order(lib, backend, nf):
    """1. A and B are both redundant only while the other's observations count: five key frames hold every point (nObs 5: four others), so after
    one cull only three others remain.  Order A, B culls A only; order B, A culls B only."""
    M = shared_world(2, nf, n_extra=3)
    exp, fin = run_and_check(lib, backend, M, [problem(4, [0, 1]), problem(4, [1, 0])], variants=["parallel"], apply=0)
    assert codes(exp[0]) == [CULL_CODE_CULLED, CULL_CODE_KEPT] and exp[0]["events"] == [(0, -1, -1)]
    assert codes(exp[1]) == [CULL_CODE_CULLED, CULL_CODE_KEPT] and exp[1]["events"] == [(1, -1, -1)]
    assert exp[0]["nred"] == [nf, 0] and fin[0].kfs[0]["bad"] and not fin[0].kfs[1]["bad"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_point_goes_bad(lib, backend):
    """2. a point with nObs == 3 in a culled key frame goes bad; the later candidate's nMPs drops from 10 to 9 and flips it to redundant (9 > 8.1f
    against 9 > 9.0f); the point's rows in the other key frames are -1 after apply"""
    good = list(range(19))
    # point 19 is seen by A (0), B (1) and key frame 2 only; A is redundant outright (19 > 18.0f), B holds nine of the good points
    kfs = [KF(good + [19]), KF(good[:9] + [19])] + [KF(good + ([19] if i == 0 else [])) for i in range(4)]
    M = Map(kfs, 20)
    exp, fin = run_and_check(lib, backend, M, [problem(5, [0, 1]), problem(5, [1])], variants=["never_bad"], apply=0)
    assert codes(exp[0]) == [CULL_CODE_CULLED, CULL_CODE_CULLED] and exp[0]["nmps"] == [20, 9] and exp[0]["nred"] == [19, 9]
    assert codes(exp[1]) == [CULL_CODE_KEPT] and exp[1]["nmps"] == [10] and exp[1]["nred"] == [9]
    assert fin[0].mps[19]["bad"] and fin[0].kfs[2]["mp"][19] is None and fin[0].kfs[1]["mp"][9] is None and fin[0].kfs[0]["mp"][19] == 19


@pytest.mark.parametrize("backend", BACKENDS)
def test_stereo_weight(lib, backend):
    """3. two stereo observations (nObs == 4) but only one other key frame: the point enters the walk and is not redundant; erasing a stereo
    observation subtracts 2, so the point (4 -> 2) goes bad"""
    common = list(range(10))
    kfs = [KF(common + [10], stereo=[False] * 10 + [True]), KF(common + [10], stereo=[False] * 10 + [True])] + [KF(common) for _ in range(4)]
    M = Map(kfs, 11)
    assert M.mps[10]["nObs"] == 4
    exp, fin = run_and_check(lib, backend, M, [problem(5, [0, 1])], variants=["weight_one"], apply=0, pass_nobs=False)
    assert exp[0]["nmps"] == [11, 10] and exp[0]["nred"] == [10, 10] and codes(exp[0]) == [CULL_CODE_CULLED, CULL_CODE_CULLED]
    assert fin[0].mps[10]["bad"] and fin[0].mps[10]["nObs"] == 2


@pytest.mark.parametrize("backend", BACKENDS)
def test_octave_gate_and_threshold_of_three(lib, backend):
    """4. the gate counts a record at the feature's octave + 1 and not at + 2; exactly 3 qualifying records are not enough, 4 are"""
    def world(other_octaves):
        return Map([KF([0, 1, 2], octave=[2, 2, 2])] + [KF([0, 1, 2], octave=[o] * 3) for o in other_octaves], 3)
    exp, _ = run_and_check(lib, backend, world([3, 3, 3, 3, 4, 4]), [problem(6, [0])], variants=["octave_zero"])
    assert codes(exp[0]) == [CULL_CODE_CULLED] and exp[0]["nred"] == [3]
    exp, _ = run_and_check(lib, backend, world([3, 3, 3, 4, 4, 4]), [problem(6, [0])], variants=["octave_two", "three_enough"])
    assert codes(exp[0]) == [CULL_CODE_KEPT] and exp[0]["nred"] == [0] and exp[0]["nmps"] == [3]


def _ratio_world(n_mps, n_red, close=None, n_obs=5):
    """key frame 0 holds n_mps points of which the first n_red are seen by n_obs other key frames, the rest by 1"""
    pts = list(range(n_mps))
    return Map([KF(pts, close=close)] + [KF(pts[:n_red] if i else pts) for i in range(n_obs)], n_mps)


@pytest.mark.parametrize("backend", BACKENDS)
def test_float_threshold_and_close(lib, backend):
    """5. nMPs = 10, nRed = 9: 0.9f * 10.0f rounds to 9.0f and the key frame is KEPT (the double product 9.000000357 would cull it); nRed = 10 is
    culled; 0.5f with nMPs = 4, nRed = 2 is kept; CLOSE is ignored under MONOCULAR and honoured otherwise"""
    assert np.float32(0.9) * np.float32(10) == np.float32(9) and float(np.float32(0.9)) * 10 < 9.0000004
    exp, _ = run_and_check(lib, backend, _ratio_world(10, 9), [problem(5, [0])], variants=["double_th"])
    assert codes(exp[0]) == [CULL_CODE_KEPT] and (exp[0]["nmps"], exp[0]["nred"]) == ([10], [9])
    exp, _ = run_and_check(lib, backend, _ratio_world(10, 10), [problem(5, [0])])
    assert codes(exp[0]) == [CULL_CODE_CULLED]
    # 0.5f: the inertial stereo threshold; 22 key frames in the map, no links, so a redundant key frame ends as KEPT_NO_NEIGHBOUR
    W = _ratio_world(4, 2)
    exp, _ = run_and_check(lib, backend, W, [problem(5, [0], inertial=True, n_in_map=30)])
    assert codes(exp[0]) == [CULL_CODE_KEPT] and (exp[0]["nmps"], exp[0]["nred"]) == ([4], [2])
    exp, _ = run_and_check(lib, backend, _ratio_world(4, 3), [problem(5, [0], inertial=True, n_in_map=30)])
    assert codes(exp[0]) == [CULL_CODE_KEPT_NO_NEIGHBOUR]
    exp, _ = run_and_check(lib, backend, _ratio_world(4, 3), [problem(5, [0], inertial=True, mono=True, n_in_map=30)])
    assert codes(exp[0]) == [CULL_CODE_KEPT]   # 0.9f again under MONOCULAR
    # CLOSE: the far feature is the one that is not redundant
    close = [True] * 9 + [False]
    exp, _ = run_and_check(lib, backend, _ratio_world(10, 9, close), [problem(5, [0]), problem(5, [0], mono=True)],
                           variants=["close_never"])
    assert codes(exp[0]) == [CULL_CODE_CULLED] and exp[0]["nmps"] == [9]
    assert codes(exp[1]) == [CULL_CODE_KEPT] and exp[1]["nmps"] == [10]
    exp, _ = run_and_check(lib, backend, _ratio_world(10, 9, close), [problem(5, [0], mono=True)], variants=["close_always"])


@pytest.mark.parametrize("backend", BACKENDS)
def test_duplicates_and_missing_records(lib, backend):
    """6. a point held by two features of one key frame counts twice in nMPs but its observation is erased once; a feature whose point has no
    record of the key frame changes nothing"""
    common = list(range(30))
    kfs = [KF(common + [30, 30, 31])] + [KF(common + [30, 31]) for _ in range(3)] + [KF(common), KF(common)]
    M = Map(kfs, 32, no_obs={(0, 31)})
    assert M.mps[30]["nObs"] == 4 and M.mps[31]["nObs"] == 3 and 0 not in M.mps[31]["obs"]
    exp, fin = run_and_check(lib, backend, M, [problem(5, [0])], variants=["dup_twice"], apply=0)
    assert codes(exp[0]) == [CULL_CODE_CULLED] and exp[0]["nmps"] == [33] and exp[0]["nred"] == [30]
    assert fin[0].mps[30]["nObs"] == 3 and not fin[0].mps[30]["bad"] and fin[0].mps[31]["nObs"] == 3 and not fin[0].mps[31]["bad"]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("abort", [False, True])
def test_break_rule(lib, backend, abort):
    """7. the break test sits at the bottom of the body: 104 candidates of 3 features with #101 and #102 bad (their `continue` skips the test) and
    #103 redundant: #103 is culled, #104 is not visited.  With ABORT_BA the same happens at 24 candidates (count > 20)."""
    n = 24 if abort else 104
    kfs = [KF([3 * i, 3 * i + 1, 3 * i + 2]) for i in range(n - 4)]
    s = 3 * (n - 4)
    kfs += [KF([s, s + 1, s + 2], bad=i < 2) for i in range(4 + 4)]
    M = Map(kfs, s + 3)
    exp, fin = run_and_check(lib, backend, M, [problem(n + 3, list(range(n)), abort=abort)], variants=["break_top"])
    assert codes(exp[0]) == [CULL_CODE_KEPT] * (n - 4) + [CULL_CODE_SKIPPED] * 2 + [CULL_CODE_CULLED, CULL_CODE_NOT_VISITED]
    assert exp[0]["events"] == [(n - 2, -1, -1)]
    if abort:   # without the flag nothing ends the loop at 24 candidates
        exp, _ = run_and_check(lib, backend, M, [problem(n + 3, list(range(n)))])
        assert codes(exp[0])[-2:] == [CULL_CODE_CULLED, CULL_CODE_CULLED]


def inertial_world(n_kf=30, dt=1.0, nf=5, spread=1.0):
    """a chain of key frames that all hold the same points (each is redundant), ids = indices, dt seconds and `spread` metres apart"""
    kfs = [KF(range(nf), ts=100.0 + dt * i, pos=(spread * i, 0.0, 0.0), prev=i - 1 if i else None, next=i + 1 if i + 1 < n_kf else None)
           for i in range(n_kf)]
    return Map(kfs, nf)


@pytest.mark.parametrize("backend", BACKENDS)
def test_inertial_exits(lib, backend):
    """8. one case per exit of :1280-1310"""
    iner = dict(inertial=True, mono=True)
    # <= 21 reached mid-walk: 22 key frames in the map, the first cull leaves 21
    M = inertial_world(dt=0.2)
    exp, _ = run_and_check(lib, backend, M, [problem(29, [3, 5], n_in_map=22, **iner)], variants=["static_count"], apply=0)
    assert codes(exp[0]) == [CULL_CODE_CULLED_IMU1, CULL_CODE_KEPT_FEW_KFS] and exp[0]["events"] == [(3, 2, 4)] and exp[0]["n_in_map"] == 21
    # the recent-id test: mnId > current - 2; with the current id 1 the unsigned difference wraps and the test is never true
    exp, _ = run_and_check(lib, backend, M, [problem(29, [28, 27], **iner)])
    assert codes(exp[0]) == [CULL_CODE_KEPT_RECENT, CULL_CODE_CULLED_IMU1]
    M1 = inertial_world(dt=0.2)
    M1.kfs[29]["id"] = 1
    for i in range(29):
        M1.kfs[i]["id"] = 100 + i
    exp, _ = run_and_check(lib, backend, M1, [problem(29, [28, 26], **iner)], variants=["signed_id"])
    assert codes(exp[0]) == [CULL_CODE_CULLED_IMU1] * 2
    # a missing neighbour (the chain's first key frame); the break test is still reached: with ABORT_BA it ends the loop at #21, while the
    # `continue` of KEPT_RECENT at #21 does not
    M = inertial_world(dt=5.0)
    exp, _ = run_and_check(lib, backend, M, [problem(29, [0], **iner)])
    assert codes(exp[0]) == [CULL_CODE_KEPT_NO_NEIGHBOUR]
    far = [1] * 20   # twenty visits of one key frame that stays (t = 10, 1 m apart)
    exp, _ = run_and_check(lib, backend, M, [problem(29, far + [0, 2], abort=True, **iner), problem(29, far + [28, 2], abort=True, **iner)])
    assert codes(exp[0])[-3:] == [CULL_CODE_KEPT_INERTIAL, CULL_CODE_KEPT_NO_NEIGHBOUR, CULL_CODE_NOT_VISITED]
    assert codes(exp[1])[-3:] == [CULL_CODE_KEPT_INERTIAL, CULL_CODE_KEPT_RECENT, CULL_CODE_KEPT_INERTIAL]
    # the first branch by each disjunct: last_ID is the id 21 links back from the current key frame (29 -> 8)
    M = inertial_world(dt=1.0)   # t = 2
    exp, _ = run_and_check(lib, backend, M, [problem(29, [7, 8, 9], imu_init=True, **iner), problem(29, [7], **iner)])
    assert codes(exp[0]) == [CULL_CODE_CULLED_IMU1, CULL_CODE_KEPT_INERTIAL, CULL_CODE_KEPT_INERTIAL]   # 7 < 8; 8 and 9 are not
    assert codes(exp[1]) == [CULL_CODE_KEPT_INERTIAL]
    M = inertial_world(dt=1.6)   # t = 3.2: not < 3
    exp, _ = run_and_check(lib, backend, M, [problem(29, [7], imu_init=True, **iner)])
    assert codes(exp[0]) == [CULL_CODE_KEPT_INERTIAL]
    M = inertial_world(dt=0.2)   # t = 0.4 < 0.5
    exp, _ = run_and_check(lib, backend, M, [problem(29, [20], **iner)])
    assert codes(exp[0]) == [CULL_CODE_CULLED_IMU1]
    # the second branch: within 0.02 m of the previous key frame, t < 3, no second inertial BA yet.  The norm is compared as a double:
    # a distance of exactly 0.02f is below 0.02 (as floats the two are equal)
    M = inertial_world(dt=1.0, spread=np.float32(0.02))
    exp, _ = run_and_check(lib, backend, M, [problem(29, [1], **iner), problem(29, [1], ba2=True, **iner)], variants=["float_norm"])
    assert codes(exp[0]) == [CULL_CODE_CULLED_IMU2] and exp[0]["events"] == [(1, 0, 2)] and codes(exp[1]) == [CULL_CODE_KEPT_INERTIAL]
    M = inertial_world(dt=1.0, spread=0.021)
    exp, _ = run_and_check(lib, backend, M, [problem(29, [10], **iner)])
    assert codes(exp[0]) == [CULL_CODE_KEPT_INERTIAL]
    M = inertial_world(dt=1.6, spread=0.001)
    exp, _ = run_and_check(lib, backend, M, [problem(29, [10], **iner)])
    assert codes(exp[0]) == [CULL_CODE_KEPT_INERTIAL]   # t = 3.2
    # a relink lengthens a later candidate's t past 0.5: 10 goes (t = 0.4), then 11 spans 9 .. 12 (t = 0.6)
    M = inertial_world(dt=0.2)
    exp, fin = run_and_check(lib, backend, M, [problem(29, [10, 11, 13]), problem(29, [10, 11, 13], **iner)], apply=1)
    assert codes(exp[1]) == [CULL_CODE_CULLED_IMU1, CULL_CODE_KEPT_INERTIAL, CULL_CODE_CULLED_IMU1]
    assert exp[1]["events"] == [(10, 9, 11), (13, 12, 14)] and fin[1].kfs[11]["prev"] == 9 and fin[1].kfs[9]["next"] == 11
    w = ref_keyframe_culling(copy.deepcopy(M), problem(29, [10, 11, 13], **iner), variant="static_links")
    assert w["code"][1] == CULL_CODE_CULLED_IMU1   # the wrong variant (links as they were at the start) culls 11 too


@pytest.mark.parametrize("backend", BACKENDS)
def test_not_erase(lib, backend):
    """8. NOT_ERASE in both modes: the decision is reported as deferred, the inertial relink has happened and is in the event, and no map state
    changes: the next candidate still sees the deferred key frame's observations"""
    M = shared_world(2, 5, n_extra=3)
    M.kfs[0]["not_erase"] = True
    exp, fin = run_and_check(lib, backend, M, [problem(4, [0, 1])], apply=0)
    assert codes(exp[0]) == [CULL_CODE_CULLED | CULL_CODE_DEFERRED, CULL_CODE_CULLED] and exp[0]["events"] == [(0, -1, -1), (1, -1, -1)]
    assert fin[0].kfs[0]["to_be_erased"] and not fin[0].kfs[0]["bad"] and all(0 in m["obs"] for m in fin[0].mps)
    M = inertial_world(dt=0.2)
    M.kfs[10]["not_erase"] = True
    exp, fin = run_and_check(lib, backend, M, [problem(29, [10, 11], n_in_map=22, inertial=True, mono=True)], apply=0)
    assert codes(exp[0]) == [CULL_CODE_CULLED_IMU1 | CULL_CODE_DEFERRED, CULL_CODE_KEPT_INERTIAL] and exp[0]["events"] == [(10, 9, 11)]
    assert exp[0]["n_in_map"] == 22 and fin[0].kfs[10]["prev"] is None and fin[0].kfs[11]["prev"] == 9 and not fin[0].kfs[10]["bad"]


def _without(M0, kf_feature=None):
    """the map as the kernel treats a damaged one: the named feature holds no point"""
    def f(M):
        M = copy.deepcopy(M)
        if kf_feature:
            k, i = kf_feature
            p = M.kfs[k]["mp"][i]
            M.kfs[k]["mp"][i] = None
            if p is not None and M.mps[p]["obs"].get(k) == i:
                del M.mps[p]["obs"][k]
        return M
    return f


@pytest.mark.parametrize("backend", BACKENDS)
def test_bad_indices(lib, backend):
    """9. indices out of range of every kind: the flag is set, the output is otherwise as if the thing were absent, nothing is read through (the
    emulated build runs on exact-size host arrays).  A rig record sets UNSUPPORTED."""
    M = shared_world(2, 6, n_extra=4)
    P = [problem(5, [0, 1])]
    clean, _ = run_and_check(lib, backend, M, P)
    assert codes(clean[0]) == [CULL_CODE_CULLED, CULL_CODE_CULLED]

    def run(corrupt, absent=None, flags=CULL_BAD_INDEX, probs=P):
        return run_and_check(lib, backend, M, probs, corrupt=corrupt, absent=absent, expect_flags=flags)[0]

    # a candidate out of range / an empty slot: skipped
    Mb = copy.deepcopy(M)
    Mb.kfs[2]["bad"] = True
    want = ref_keyframe_culling(copy.deepcopy(Mb), problem(5, [2, 1]))
    m = orbhip.ORBmatcher(0.8, True, lib=lib)
    view, cull, ref, owner = flatten(M)
    pr, cands = problems_array(M, [problem(5, [2, 1])])
    for bad in (99, -1, -7):
        c2 = cands.copy()
        c2[0] = bad
        dv, dc = dev_view(view, cull, backend)
        out = m.CullKeyFrames(dv, dc, to_dev(pr, backend), to_dev_plain(c2, backend), 4, n_cand_max=2, out=sentinel_out(1, 4, backend))
        sync(backend)
        assert list(to_host(out["code"])[0][:2]) == [CULL_CODE_SKIPPED, want["code"][1]] and int(to_host(out["flags"])[0]) == CULL_BAD_INDEX
        assert list(to_host(out["nmps"])[0][:2]) == [0, want["nmps"][1]]

    # a d_kf_mp entry out of range, and one that names a slot that is not VALID: the feature holds no point
    def entry(val):
        def f(v, c, pr, cands):
            v["kf_mp"][int(v["kf"][0]["mp_row0"]) + 2] = val
        return f
    for val in (6, -3, 1 << 30):
        e = run(entry(val), absent=_without(M, kf_feature=(0, 2)))
        # the point's record of key frame 0 is still in the CSR: the restatement drops it with the feature, the kernel never reaches it, and the
        # outputs compared here (codes, counts, events) agree
        assert e[0]["nmps"] == [5, 6]

    def invalid_slot(v, c, pr, cands):
        v["mp"]["flags"][2] = 0

    def no_point_2(M_):
        M_ = copy.deepcopy(M_)
        for k in M_.kfs:
            k["mp"][2] = None
        M_.mps[2]["obs"] = {}
        return M_
    e = run(invalid_slot, absent=no_point_2)
    assert e[0]["nmps"] == [5, 5]

    # a record's kf out of range, a feature index (desc_row) outside the key frame: the record is absent
    def rec_kf(v, c, pr, cands):
        v["obs"]["kf"][int(v["obs_start"][3]) + 4] = 77   # point 3's record of key frame 4

    def no_record(M_):
        M_ = copy.deepcopy(M_)
        del M_.mps[3]["obs"][4]
        return M_
    e = run(rec_kf, absent=no_record)
    assert codes(e[0]) == [CULL_CODE_CULLED, CULL_CODE_KEPT] and e[0]["nred"] == [6, 5]   # point 3 has one observer less

    def rec_row(v, c, pr, cands):
        v["obs"]["desc_row"][int(v["obs_start"][3]) + 4] = int(c["ckf"][4]["desc_row0"]) + 6
    run(rec_row, absent=no_record)

    def rec_right(v, c, pr, cands):
        v["obs"]["flags"][int(v["obs_start"][3]) + 4] = OBS_RIGHT
    run(rec_right, absent=no_record, flags=CULL_UNSUPPORTED)

    # a CSR range that leaves [0, n_obs]: the point is absent
    def csr(v, c, pr, cands):
        v["obs_start"][3] = len(v["obs"]) + 9

    def no_point_23(M_):   # obs_start[3] bounds point 2 (its end) and point 3 (its start)
        M_ = copy.deepcopy(M_)
        for k in M_.kfs:
            k["mp"][2] = k["mp"][3] = None
        M_.mps[2]["obs"], M_.mps[3]["obs"] = {}, {}
        return M_
    e = run(csr, absent=no_point_23)
    assert e[0]["nmps"] == [4, 4]

    # a key frame's rows past the table: no features
    def rows(v, c, pr, cands):
        v["kf"][1]["n_feat"] = len(v["kf_mp"])

    def no_features_1(M_):
        M_ = copy.deepcopy(M_)
        for p, i in enumerate(range(6)):
            del M_.mps[p]["obs"][1]
        M_.kfs[1]["mp"] = [None] * 6
        return M_
    e = run(rows, absent=no_features_1)
    assert e[0]["nmps"] == [6, 0] and codes(e[0]) == [CULL_CODE_CULLED, CULL_CODE_KEPT]

    # the current key frame or the candidate range cannot be read: nothing is visited
    def cur(v, c, pr, cands):
        pr[0]["current_kf"] = 9
    run(cur, absent=lambda M_: M_, probs=[problem(5, [])])
    for field, val in (("current_kf", 9), ("cand_start", -1), ("n_cand", 3), ("cand_start", 1)):
        pr2 = pr.copy()
        pr2[0][field] = val
        dv, dc = dev_view(view, cull, backend)
        out = m.CullKeyFrames(dv, dc, to_dev(pr2, backend), to_dev_plain(cands, backend), 4, n_cand_max=2, out=sentinel_out(1, 4, backend))
        sync(backend)
        n_written = 2 if field == "current_kf" else 0
        assert list(to_host(out["code"])[0]) == [0] * n_written + [SENT8] * (4 - n_written), field
        assert int(to_host(out["flags"])[0]) == CULL_BAD_INDEX and int(to_host(out["n_events"])[0]) == 0

    # links: out of range or an empty slot -> no neighbour
    Mi = inertial_world(dt=0.2)

    def link(v, c, pr, cands):
        c["ckf"][10]["next"] = 44

    def no_next(M_):
        M_ = copy.deepcopy(M_)
        M_.kfs[10]["next"] = None
        return M_
    e = run_and_check(lib, backend, Mi, [problem(29, [10], inertial=True, mono=True)], corrupt=link, absent=no_next, expect_flags=CULL_BAD_INDEX)[0]
    assert codes(e[0]) == [CULL_CODE_KEPT_NO_NEIGHBOUR]


@pytest.mark.parametrize("backend", BACKENDS)
def test_more_features_than_lanes_and_batch(lib, backend):
    """10. a candidate with WG + 1 features, where the count of the last feature decides (the greatest nRed that is not above 0.9f * nMPs is
    kept, one more is culled); batch = 3 with different candidate orders on one view: independent results"""
    n = WG + 1
    most = int(np.floor(np.float32(0.9) * np.float32(n)))
    assert np.float32(most) <= np.float32(0.9) * np.float32(n) < np.float32(most + 1)
    for n_red, want in ((most, CULL_CODE_KEPT), (most + 1, CULL_CODE_CULLED)):
        exp, _ = run_and_check(lib, backend, _ratio_world(n, n_red), [problem(5, [0])])
        assert codes(exp[0]) == [want] and exp[0]["nmps"] == [n] and exp[0]["nred"] == [n_red]
    M = shared_world(3, 9, n_extra=2)   # five holders: any one cull leaves the others at three other observers
    exp, _ = run_and_check(lib, backend, M, [problem(4, [0, 1, 2]), problem(4, [2, 1, 0]), problem(4, [1, 1, 0])], apply=1)
    assert [e["events"] for e in exp] == [[(0, -1, -1)], [(2, -1, -1)], [(1, -1, -1)]]
    assert codes(exp[2]) == [CULL_CODE_CULLED, CULL_CODE_SKIPPED, CULL_CODE_KEPT]   # the second visit finds it bad


# ------------------------------------------------------------------------------------------------ fuzz
def random_world(rng, inertial):
    """at most 12 key frames x 70 features over at most 300 points: a core of points most key frames see (so that some key frames are
    redundant), fringe points with three observers (so that a cull makes points go bad), duplicates inside a key frame (drawn with
    replacement), a random pointer order; the key frames form the inertial chain"""
    n_kf = int(rng.integers(9, 13))
    n_core = int(rng.integers(25, 41))
    n_fringe = int(rng.integers(10, 40))
    n_mp = n_core + n_fringe
    holders = [[int(x) for x in rng.choice(n_kf, 3, replace=False)] for _ in range(n_fringe)]
    order = [int(x) for x in rng.permutation(n_kf)]
    kfs = []
    for k in range(n_kf):
        nf = int(rng.integers(20, 71))
        p_fringe = float(rng.choice([0.0, 0.04, 0.1]))
        mine = [n_core + j for j, h in enumerate(holders) if k in h]
        mp = []
        for _ in range(nf):
            u = rng.random()
            mp.append(int(rng.choice(mine)) if (u < p_fringe and mine) else (None if u > 0.9 else int(rng.integers(0, n_core))))
        lo, hi = (1, 3) if rng.random() < 0.7 else (0, 4)
        kfs.append(KF(mp, octave=[int(x) for x in rng.integers(lo, hi, nf)], close=[bool(x) for x in rng.random(nf) < 0.9],
                      stereo=[bool(x) for x in rng.random(nf) < 0.3], bad=bool(rng.random() < 0.05), not_erase=bool(rng.random() < 0.08),
                      ts=50.0 + 0.22 * k + float(rng.random()) * 0.1, pos=tuple(float(x) for x in rng.normal(0, 0.008 if k % 3 else 1.0, 3)),
                      prev=k - 1 if k else None, next=k + 1 if k + 1 < n_kf else None, id=10 + 2 * k))
    bad_mp = [p for p in range(n_mp) if rng.random() < 0.03]
    M = Map(kfs, n_mp, order=order, bad_mp=bad_mp)
    cur = n_kf - 1
    cands = [int(x) for x in rng.permutation(n_kf - 1)]
    P = problem(cur, cands, init_id=10, n_in_map=int(rng.integers(21, 28)) if inertial else None, inertial=inertial,
                mono=bool(rng.random() < 0.5), imu_init=bool(rng.random() < 0.5), ba2=bool(rng.random() < 0.3))
    return M, P


FUZZ_SEEDS = list(range(1000, 1024))


def test_fuzz_seed_set_is_not_vacuous():
    """from the restatement alone: at least half of the seeds cull two or more key frames, a quarter make a point go bad, a quarter take an
    inertial relink"""
    culls = bad = relink = 0
    for seed in FUZZ_SEEDS:
        rng = np.random.default_rng(seed)
        M, P = random_world(rng, inertial=bool(seed & 1))
        before = sum(m["bad"] for m in M.mps)
        e = ref_keyframe_culling(M, P)
        erased = [c for c in e["code"] if c in (CULL_CODE_CULLED, CULL_CODE_CULLED_IMU1, CULL_CODE_CULLED_IMU2)]
        culls += len(erased) >= 2
        bad += sum(m["bad"] for m in M.mps) > before
        relink += any(ev[1] >= 0 for ev in e["events"])
    n = len(FUZZ_SEEDS)
    assert culls * 2 >= n and bad * 4 >= n and relink * 4 >= n, (culls, bad, relink, n)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz(lib, backend, seed):
    rng = np.random.default_rng(seed)
    M, P = random_world(rng, inertial=bool(seed & 1))
    P2 = dict(P, cands=list(reversed(P["cands"])))
    run_and_check(lib, backend, M, [P, P2], apply=seed % 2, pass_nobs=bool(seed & 2))


def test_reversed_lane_order():
    """the emulated build under EMU_REVERSE=1 (lanes scheduled in reverse): the compare-and-swap makes every record die once whatever the order"""
    env = dict(os.environ, EMU_REVERSE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", __file__, "-k",
                        "emu and (test_duplicates or test_point_goes_bad or test_stereo_weight or (test_fuzz and (1001 or 1002 or 1003 or 1004)))"],
                       env=env, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ apply: overflow
@pytest.mark.parametrize("backend", BACKENDS)
def test_apply_overflow_and_exact_fit(lib, backend):
    """12. obs_out one record short: the need is reported, the overflow flag set and nothing written; an exact fit is written"""
    M = shared_world(2, 7, n_extra=3)
    exp, fin = run_and_check(lib, backend, M, [problem(4, [0, 1])], apply=0, cap_obs_out=7 * 4 - 1)
    run_and_check(lib, backend, M, [problem(4, [0, 1])], apply=0, cap_obs_out=7 * 4)
    # an empty map (every count 0): the current key frame cannot be read, nothing is visited, the compacted CSR is the single 0
    E = Map([], 0)
    view, cull, ref, _ = flatten(E)
    m = orbhip.ORBmatcher(0.8, True, lib=lib)
    dv, dc = dev_view(view, cull, backend)
    pr = np.zeros(1, CULL_PROBLEM_DTYPE)
    out = m.CullKeyFrames(dv, dc, to_dev(pr, backend), to_dev_plain(np.zeros(0, np.int32), backend), 2, n_cand_max=0, out=sentinel_out(1, 2, backend))
    app = m.ApplyKeyFrameCulling(dv, dc, out, rec_dev(ref, backend), 0)
    sync(backend)
    assert int(to_host(out["flags"])[0]) == CULL_BAD_INDEX and int(to_host(out["n_events"])[0]) == 0 and np.all(to_host(out["code"]) == SENT8)
    assert list(to_host(app["result"])) == [0, 0] and list(to_host(app["obs_start"])) == [0]


@pytest.mark.parametrize("backend", BACKENDS)
def test_apply_scans_more_than_256_blocks(lib, backend):
    """13. 65 536 + 300 points, nearly all without records: 258 blocks of 256 points, so the one-workgroup scan of the block totals takes a
    second chunk, whose offsets continue the first's.  The points with records sit in a few blocks on both sides of block 256; five key frames
    hold them all, so the first candidate is culled (and its records leave the CSR) and the second kept"""
    pts = [3, 4, 300, 301, 302, 20000, 65530, 65535, 65536, 65537, 65800, 65801, 65835]
    M = Map([KF(pts) for _ in range(5)], 65536 + 300)
    exp, fin = run_and_check(lib, backend, M, [problem(4, [0, 1])], apply=0)
    assert codes(exp[0]) == [CULL_CODE_CULLED, CULL_CODE_KEPT] and sum(len(x["obs"]) for x in fin[0].mps) == 4 * len(pts)


def test_flatten_cull_keyframes():
    """CLOSE with the reference's expression (a NaN depth is close: both comparisons are false), STEREO = mvuRight >= 0, rigs refused"""
    k = dict(mp=[0, 1, 2, 3], octave=[0, 3, 7, 1], depth=[1.0, 40.0, -1.0, float("nan")], th_depth=35.0, u_right=[5.0, -1.0, 0.0, -1.0], id=9,
             prev=-1, next=-1, timestamp=2.5, imu_pos=(1, 2, 3), not_erase=True)
    ckf, feat = flatten_cull_keyframes([None, k])
    assert list(feat) == [0x40 | 0x80, 3, 7 | 0x80, 1 | 0x40] and ckf[1]["id"] == 9 and ckf[1]["flags"] == 1 and ckf[1]["desc_row0"] == 0
    with pytest.raises(orbhip.OrbHipError):
        flatten_cull_keyframes([dict(k, NLeft=2)])
    with pytest.raises(orbhip.OrbHipError):
        flatten_cull_keyframes([dict(k, camera2=True)])


# ------------------------------------------------------------------------------------------------ graph capture
@pytest.mark.gpu
def test_graph_capture_replay_hip(hip_lib):
    """11. cull -> apply captured on one stream and replayed twice from the same map: the same bytes both times, equal to the eager call"""
    import torch
    rng = np.random.default_rng(77)
    M, P = random_world(rng, inertial=True)
    view, cull, ref, owner = flatten(M)
    pr, cands = problems_array(M, [P, dict(P, cands=list(reversed(P["cands"])))])
    m = orbhip.ORBmatcher(0.8, True, lib=hip_lib)
    dv, dc = dev_view(view, cull, "hip")
    d_ref = to_dev(ref, "hip")
    keep = {k: v.clone() for k, v in list(dv.items()) + [("ckf", dc["ckf"]), ("mp_nobs", dc["mp_nobs"]), ("ref", d_ref)]}
    d_pr, d_c = to_dev(pr, "hip"), to_dev_plain(cands, "hip")
    cap = len(P["cands"]) + 1

    def restore():
        for k, v in keep.items():
            (dv[k] if k in dv else (d_ref if k == "ref" else dc[k])).copy_(v)

    def step(out=None, app=None):
        out = m.CullKeyFrames(dv, dc, d_pr, d_c, cap, out=out)
        app = m.ApplyKeyFrameCulling(dv, dc, out, d_ref, len(view["obs"]), problem=1, out=app)
        return out, app

    def snapshot(out, app):
        torch.cuda.synchronize()
        state = [v for b in range(2) for _, v in sorted(m.CullState(dv, out, b).items())]   # (the sections; the padding between them is nobody's)
        return [out[k].cpu().numpy().copy() for k in ("code", "nmps", "nred", "events", "n_events", "flags")] + state + \
            [app[k].cpu().numpy().copy() for k in ("obs_start", "obs", "result")] + \
            [x.cpu().numpy().copy() for x in (dv["mp"], dv["kf"], dv["kf_mp"], dc["ckf"], dc["mp_nobs"], d_ref)]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out, app = step()   # allocates the outputs and the workspace outside the capture
    torch.cuda.current_stream().wait_stream(s)
    eager = snapshot(out, app)
    assert eager[4].sum() >= 1
    restore()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(out, app)
    for r in range(2):
        restore()
        out["work"].fill_(0x77)
        torch.cuda.synchronize()
        g.replay()
        got = snapshot(out, app)
        for i, (x, y) in enumerate(zip(got, eager)):
            assert np.array_equal(x, y), (r, i)


# ------------------------------------------------------------------------------------------------ sizes and refusals
def test_workspace_bytes(emu_lib):
    """13. orbm_cull_workspace_bytes over zero, negative and odd arguments against the layout walked here: hdr int32[8] | nobs int32[n_mp] |
    rec uint32[n_obs] | prev, next int32[n_kf] | blk int32[ceil(n_mp / 256) + 1] | mp_bad uint8[n_mp] | kf_erased uint8[n_kf], every section
    padded to 16 bytes"""
    L = emu_lib
    pad = lambda n: (n + 15) & ~15   # noqa: E731
    for n_kf, n_mp, n_obs, batch in [(0, 0, 0, 1), (1, 1, 1, 1), (5, 7, 9, 2), (12, 300, 4001, 3), (101, 6001, 120007, 64), (3, 257, 5, 1),
                                     (3, 256, 5, 7), (17, 0, 0, 0)]:
        secs = [32, pad(4 * n_mp), pad(4 * n_obs), pad(4 * n_kf), pad(4 * n_kf), pad(4 * ((n_mp + 255) // 256 + 1)), pad(n_mp), pad(n_kf)]
        assert L.orbm_cull_workspace_bytes(n_kf, n_mp, n_obs, batch) == batch * sum(secs) and sum(secs) % 16 == 0
        Y = CullWorkspaceLayout()
        assert L.orbm_cull_workspace(n_kf, n_mp, n_obs, C.byref(Y)) == 0
        off = np.cumsum([0] + secs)
        assert (Y.stride, Y.nobs, Y.rec, Y.prev, Y.next, Y.mp_bad, Y.kf_erased) == (sum(secs), off[1], off[2], off[3], off[4], off[6], off[7])
    for a in [(-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1)]:
        assert L.orbm_cull_workspace_bytes(*a) == 0
    assert L.orbm_cull_workspace(-1, 1, 1, C.byref(Y)) == ORB_E_INVALID and L.orbm_cull_workspace(1, 1, 1, None) == ORB_E_INVALID


@pytest.mark.parametrize("backend", BACKENDS)
def test_argument_errors(lib, backend):
    """14. the host entries refuse null pointers, negative counts, misaligned slabs, candidates above cap_cand; batch == 0 is a no-op"""
    M = shared_world(2, 5)
    view, cull, ref, owner = flatten(M)
    pr, cands = problems_array(M, [problem(5, [0, 1])])
    m = orbhip.ORBmatcher(0.8, True, lib=lib)
    dv, dc = dev_view(view, cull, backend)
    keep = [to_dev(pr, backend), to_dev_plain(cands, backend), to_dev(ref, backend)]
    o = sentinel_out(1, 4, backend)
    work = m.CullWorkspace(dv, 1)
    a = orbhip.matcher._addr
    p = orbhip.matcher.ptr
    V0, I0 = m._cull_view(dv), m._cull_in(dv, dc, keep[0], keep[1], 2)
    from orbhip._abi import LocalMapView
    view_ = lambda: LocalMapView.from_buffer_copy(V0)   # noqa: E731
    in_ = lambda: CullIn.from_buffer_copy(I0)           # noqa: E731
    out_ = lambda: CullOut(*[a(o[k]) for k in ("code", "nmps", "nred", "events", "n_events", "flags")], 4, 0)   # noqa: E731

    def call(V=None, I=None, O=None, batch=1, wk=work):
        V, I, O = V or view_(), I or in_(), O or out_()
        return lib.orbm_cull_keyframes(C.byref(V), C.byref(I), batch, C.byref(O), p(wk), None)

    assert call() == 0 and call(batch=0) == 0
    sync(backend)
    assert call(batch=-1) == ORB_E_INVALID and call(wk=None) == ORB_E_INVALID
    assert lib.orbm_cull_keyframes(None, None, 1, None, None, None) == ORB_E_INVALID
    for name in ("d_mp", "d_obs_start", "d_obs", "d_kf", "d_kf_mp"):
        x = view_()
        setattr(x, name, None)
        assert call(V=x) == ORB_E_INVALID, name
    for name in ("n_mp", "n_obs", "n_kf", "n_kf_mp_rows"):
        x = view_()
        setattr(x, name, -1)
        assert call(V=x) == ORB_E_INVALID, name
    x = view_()
    x.d_mp = x.d_mp + 4
    assert call(V=x) == ORB_E_INVALID   # a misaligned slab
    for name in ("d_ckf", "d_feat", "d_problems", "d_candidates"):
        x = in_()
        setattr(x, name, None)
        assert call(I=x) == ORB_E_INVALID, name
    x = in_()
    x.d_mp_nobs = None
    assert call(I=x) == 0   # optional
    for name, val in (("n_candidates", -1), ("n_cand_max", -1), ("n_cand_max", 5)):   # 5 candidates above cap_cand = 4
        x = in_()
        setattr(x, name, val)
        assert call(I=x) == ORB_E_INVALID, name
    for name, _ in CullOut._fields_[:6]:
        x = out_()
        setattr(x, name, None)
        assert call(O=x) == ORB_E_INVALID, name
    x = out_()
    x.cap_cand = 0
    assert call(O=x) == ORB_E_INVALID
    sync(backend)
    # apply
    app = dict(obs_start=to_dev_plain(np.zeros(len(M.mps) + 1, np.int32), backend), obs=to_dev_plain(np.zeros((64, 12), np.uint8), backend),
               result=to_dev_plain(np.zeros(2, np.int32), backend))
    apply_ = lambda: CullApply(a(dv["mp"]), a(dv["kf"]), a(dc["ckf"]), a(dv["kf_mp"]), a(dc["mp_nobs"]), a(keep[2]), a(app["obs_start"]),  # noqa: E731
                               a(app["obs"]), a(app["result"]), 64, 0)

    def call2(Y=None, batch=1, problem_=0, wk=work, I=None):
        Y, I = Y or apply_(), I or in_()
        return lib.orbm_apply_keyframe_culling(C.byref(V0), C.byref(I), batch, problem_, C.byref(Y), p(wk), None)

    assert call2() == 0
    sync(backend)
    assert [call2(batch=-1), call2(problem_=1), call2(problem_=-1), call2(wk=None), call2(batch=0)] == [ORB_E_INVALID] * 5
    for name, _ in CullApply._fields_[:9]:
        if name == "d_mp_nobs":
            continue
        x = apply_()
        setattr(x, name, None)
        assert call2(Y=x) == ORB_E_INVALID, name
    x = apply_()
    x.cap_obs_out = -1
    assert call2(Y=x) == ORB_E_INVALID
    x = in_()
    x.d_problems = None
    assert call2(I=x) == 0   # the apply does not read the problem records
    sync(backend)
    with pytest.raises(orbhip.OrbHipError):
        m.check_cull_flags(dict(flags=np.array([0, CULL_UNSUPPORTED])))
    with pytest.raises(orbhip.OrbHipError):
        m.CullKeyFrames(dv, dc, keep[0], keep[1], 4, work=np.zeros(16, np.uint8) if backend == "emu" else work[:16], out=sentinel_out(1, 4, backend))
