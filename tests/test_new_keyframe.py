"""The head of LocalMapping::Run on the device map (include/orbhip.h "New key frame"): orbm_process_new_keyframe, orbm_recent_points_push and
orbm_cull_map_points against a literal Python restatement of LocalMapping.cc:375-411 and :435-494 with MapPoint::AddObservation
(MapPoint.cc:160-195) and MapPoint::SetBadFlag (:254-277), written over dicts and lists as the reference holds them: mObservations is a dict
walked in the rank order of the key frames (std::map<KeyFrame*, .>), the loops are serial, and ComputeDistinctiveDescriptors /
UpdateNormalAndDepth are the numpy float32 / float64 restatements of tests/test_map_refresh.py (DESIGN.md "Map-point refresh").

Every output is compared by exact equality.  Where a constructed case names a wrong variant, the case is also run through that deliberately
wrong variant OF THE RESTATEMENT, so that it is known to discriminate."""
import copy
import ctypes

import numpy as np
import pytest

from devarrays import BACKENDS, lib, to_dev, to_dev_plain, to_host  # noqa: F401
from orbhip import KP_DTYPE
from orbhip._abi import (CULL_FEAT_STEREO, CULL_KEYFRAME_DTYPE, KEYFRAME_CENTER_DTYPE, LM_KF_BAD, LM_KF_PRESENT, LOCALMAP_KEYFRAME_DTYPE,
                         MAP_POINT_DTYPE, MP_BAD, MP_HAS_OBS, MP_VALID, MPCULL_CODE_BAD_INDEX, MPCULL_CODE_CULLED_OBS, MPCULL_CODE_CULLED_RATIO,
                         MPCULL_CODE_ERASED_BAD, MPCULL_CODE_KEPT, MPCULL_CODE_RETIRED, NEW_POINT_DTYPE,
                         NEWKF_BAD_INDEX, NEWKF_CODE_ADDED, NEWKF_CODE_BAD_INDEX, NEWKF_CODE_BAD_POINT, NEWKF_CODE_NONE,
                         NEWKF_CODE_PUSHED, NEWKF_CODE_PUSHED_DUP, NEWKF_OBS_OVERFLOW, NEWKF_R_FLAGS, NEWKF_R_N_ADDED, NEWKF_R_N_OBS,
                         NEWKF_R_N_PUSH_REQUIRED, NEWKF_R_N_PUSHED, NEWKF_RECENT_OVERFLOW, NEWKF_REFRESH_OVERFLOW, NEWKF_UNSORTED,
                         NEWKF_UNSUPPORTED, NEWPT_PAIR_DTYPE, OBS_KF_BAD, OBS_RIGHT, OBSERVATION_DTYPE, ORB_E_CAPACITY, ORB_E_INVALID,
                         REFRESH_MAX_OBS, REFRESH_POINT_DTYPE, LocalMapView, MpCullOut, NewKfIn, NewKfOut, RefreshParams)
from orbhip._lib import OrbHipError, ptr
from orbhip.new_keyframe import NewKeyFrame
from test_map_refresh import distinctive, normal_and_depth

f32 = np.float32
NLEVELS = 8
SF = np.ones(NLEVELS, np.float32)
for _i in range(1, NLEVELS):
    SF[_i] = SF[_i - 1] * f32(1.2)
WG = 256   # the lanes of a workgroup of csrc/orbm_newkeyframe.hip: features, list entries and points are taken 256 at a time


# ------------------------------------------------------------------------------------------------ a map as the reference holds it
def desc_of(key, flips=()):
    """a 32-byte descriptor: the pattern of `key` with the bits `flips` inverted"""
    d = np.random.default_rng(1000 + key).integers(0, 256, 32, dtype=np.uint8)
    for b in flips:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def KF(mp, stereo=None, desc=None, center=(0.0, 0.0, 0.0), oct=None, **kw):
    """one key frame: mp = GetMapPointMatches() as point indices (None = null); desc: one row per feature (default: a pattern per feature)"""
    n = len(mp)
    d = dict(id=None, bad=False, mp=list(mp), stereo=list(stereo) if stereo is not None else [False] * n,
             desc=np.array(desc, np.uint8).reshape(n, 32) if desc is not None else np.zeros((n, 32), np.uint8),
             center=np.asarray(center, f32), oct=list(oct) if oct is not None else [0] * n)
    d.update(kw)
    return d


def MP(pos=(0.0, 0.0, 5.0), **kw):
    d = dict(valid=True, bad=False, pos=np.asarray(pos, f32), normal=np.array([0, 0, 1], f32), min_d=f32(1), max_d=f32(9),
             desc=np.zeros(32, np.uint8), nObs=None, obs={}, found=1, visible=1, first=0, ref_kf=0, level=0)
    d.update(kw)
    d["obs"] = dict(d["obs"])
    return d


class World:
    """kfs: KF dicts (None = an empty slot); mps: MP dicts.  obs of a point = {kf: leftIndex}; nObs where not given is the weighted count.
    order = the key frames by pointer rank."""

    def __init__(self, kfs, mps, order=None):
        self.kfs, self.mps = kfs, mps
        self.order = list(order) if order is not None else list(range(len(kfs)))
        self.rank = {k: r for r, k in enumerate(self.order)}
        for i, k in enumerate(kfs):
            if k is not None and k["id"] is None:
                k["id"] = 100 + i
            if k is not None and not k["desc"].any():
                for j in range(len(k["mp"])):
                    k["desc"][j] = desc_of(1000 * i + j)
        for m in mps:
            if m["nObs"] is None:
                m["nObs"] = self.weight_sum(m)

    def weight_sum(self, m):
        return sum(2 if self.kfs[k]["stereo"][i] else 1 for k, i in m["obs"].items())

    def items(self, p, variant=None):
        """mObservations in iteration order"""
        it = sorted(self.mps[p]["obs"].items(), key=lambda e: self.rank[e[0]])
        last = self.mps[p].get("appended") if variant == "append_order" else None   # the wrong variant: the new record at the end
        return [e for e in it if e[0] != last] + [e for e in it if e[0] == last]


# ------------------------------------------------------------------------------------------------ the restatement
class Result:
    pass


def refresh(W, p, variant, R):
    """UpdateNormalAndDepth and ComputeDistinctiveDescriptors of point p (:398-400), with the rules of orbm_refresh_map_points"""
    m, items = W.mps[p], W.items(p, variant)
    usable = [(k, i) for k, i in items if not W.kfs[k]["bad"]]
    if len(usable) > REFRESH_MAX_OBS:
        R.flags |= NEWKF_REFRESH_OVERFLOW
        return
    m["normal"], m["min_d"], m["max_d"] = normal_and_depth(m["pos"], [W.kfs[k]["center"] for k, _ in items], W.kfs[m["ref_kf"]]["center"],
                                                           SF[m["level"]], SF[NLEVELS - 1])
    if usable:
        descs = np.array([W.kfs[k]["desc"][i] for k, i in usable])
        m["desc"] = descs[distinctive(descs)].copy()


def restate_process(W0, cur, recent, cap_recent, cap_obs_out, use_nobs=True, variant=None):
    """LocalMapping.cc:375-411, serially -> Result(W, code, sel, recent, flags, n_added, n_pushed, n_push_required, n_obs)"""
    W, R = copy.deepcopy(W0), Result()
    R.flags, R.code, R.sel, pushes, added = 0, [], [], [], set()
    for i, p in enumerate(W.kfs[cur]["mp"]):
        if p is None:
            R.code.append(NEWKF_CODE_NONE)
            continue
        m = W.mps[p]
        if m["bad"]:
            R.code.append(NEWKF_CODE_BAD_POINT)
        elif cur not in m["obs"]:
            if not use_nobs:
                m["nObs"] = W.weight_sum(m)
            m["obs"][cur], m["appended"] = i, cur               # AddObservation
            m["nObs"] += 2 if W.kfs[cur]["stereo"][i] else 1
            refresh(W, p, variant, R)
            R.sel.append(p)
            added.add(p)
            R.code.append(NEWKF_CODE_ADDED)
        else:
            pushes.append(p)                                    # mlpRecentAddedMapPoints.push_back
            R.code.append(NEWKF_CODE_PUSHED_DUP if p in added else NEWKF_CODE_PUSHED)
    R.n_obs = sum(len(m["obs"]) for m in W.mps if m["valid"])
    R.n_push_required = len(pushes)
    if R.n_push_required > cap_recent - len(recent):
        R.flags |= NEWKF_RECENT_OVERFLOW
    if R.n_obs > cap_obs_out:                                   # the call writes the codes and the result words only
        R.flags = (R.flags | NEWKF_OBS_OVERFLOW) & ~NEWKF_REFRESH_OVERFLOW
        R.W, R.recent, R.n_added, R.n_pushed, R.sel = copy.deepcopy(W0), list(recent), 0, 0, None
        return R
    R.W, R.n_added = W, len(R.sel)
    R.recent = (list(recent) + pushes)[:cap_recent]
    R.n_pushed = len(R.recent) - len(recent)
    return R


def found_ratio_lt_quarter(m, variant=None):
    if variant == "int_ratio":
        return 4 * m["found"] < m["visible"]
    with np.errstate(all="ignore"):
        return bool(f32(m["found"]) / f32(m["visible"]) < f32(0.25))   # static_cast<float>(mnFound) / mnVisible < 0.25f


def int32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


def restate_cull(W0, cur, recent, cap_obs_out, mono=False, use_nobs=True, variant=None):
    """LocalMapping.cc:435-494 with MapPoint::SetBadFlag, serially -> Result(W, code, recent, culled, flags, n_obs)"""
    W, R = copy.deepcopy(W0), Result()
    R.flags, R.code, R.recent, R.culled = 0, [], [], []
    cur_id, th = W.kfs[cur]["id"], 2 if mono else 3

    def set_bad(p):
        m = W.mps[p]
        m["bad"] = True
        for k, i in m["obs"].items():
            W.kfs[k]["mp"][i] = None          # EraseMapPointMatch(leftIndex), whatever the slot holds
        m["obs"] = {}
        R.culled.append(p)
    for p in recent:
        m = W.mps[p]
        diff = int32(int32(cur_id) - int32(m["first"]))
        n_obs = m["nObs"] if use_nobs else W.weight_sum(m)
        if m["bad"]:
            R.code.append(MPCULL_CODE_ERASED_BAD)
        elif found_ratio_lt_quarter(m, variant):
            set_bad(p)
            R.code.append(MPCULL_CODE_CULLED_RATIO)
        elif diff >= 2 and n_obs <= th:
            set_bad(p)
            R.code.append(MPCULL_CODE_CULLED_OBS)
        elif diff >= 3:
            R.code.append(MPCULL_CODE_RETIRED)
        else:
            R.recent.append(p)
            R.code.append(MPCULL_CODE_KEPT)
    R.n_obs = sum(len(m["obs"]) for m in W.mps if m["valid"])
    R.W = W
    if R.n_obs > cap_obs_out:
        R.flags |= NEWKF_OBS_OVERFLOW
        R.W = copy.deepcopy(W0)
    return R


# ------------------------------------------------------------------------------------------------ the map on the device
def flatten(W, csr=None, kf_mp_raw=None):
    """-> (view, kfs) numpy dicts for NewKeyFrame; csr: per point an explicit record list [(kf, idx, flags)] replacing the rank-ordered one
    (unsorted rows, rig records, bad indices); kf_mp_raw: {(kf, i): raw entry}"""
    n_kf, n_mp = len(W.kfs), len(W.mps)
    kf = np.zeros(n_kf, LOCALMAP_KEYFRAME_DTYPE)
    kf["parent"], kf["prev"], kf["covis"] = -1, -1, -1
    ckf, center = np.zeros(n_kf, CULL_KEYFRAME_DTYPE), np.zeros(n_kf, KEYFRAME_CENTER_DTYPE)
    rows, feat, descs = [], [], []
    for i, k in enumerate(W.kfs):
        if k is None:
            continue
        kf[i]["flags"] = LM_KF_PRESENT | (LM_KF_BAD if k["bad"] else 0)
        kf[i]["mp_row0"], kf[i]["n_feat"] = len(rows), len(k["mp"])
        ckf[i]["id"], ckf[i]["desc_row0"] = k["id"] & 0xFFFFFFFF, len(rows)
        center[i]["left"] = k["center"]
        rows += [(kf_mp_raw or {}).get((i, j), -1 if p is None else p) for j, p in enumerate(k["mp"])]
        feat += [(o & 0x3F) | (CULL_FEAT_STEREO if s else 0) for o, s in zip(k["oct"], k["stereo"])]
        descs.append(k["desc"])
    mp = np.zeros(n_mp, MAP_POINT_DTYPE)
    ref = np.zeros(n_mp, REFRESH_POINT_DTYPE)
    mp_desc = np.zeros((max(n_mp, 1), 32), np.uint8)
    recs = []
    for p, m in enumerate(W.mps):
        mp[p]["pos"], mp[p]["normal"], mp[p]["min_distance"], mp[p]["max_distance"], mp[p]["desc_row"] = m["pos"], m["normal"], m["min_d"], m["max_d"], p
        mp[p]["flags"] = (MP_VALID if m["valid"] else 0) | (MP_BAD if m["bad"] else 0) | (MP_HAS_OBS if m["nObs"] > 0 else 0)
        ref[p]["ref_kf"], ref[p]["level"] = m["ref_kf"], m["level"]
        mp_desc[p] = m["desc"]
        if csr is not None and p in csr:
            recs.append([(k, (int(ckf[k]["desc_row0"]) if 0 <= k < n_kf else 0) + i, fl) for k, i, fl in csr[p]])
        else:
            recs.append([(k, int(ckf[k]["desc_row0"]) + i, OBS_KF_BAD if W.kfs[k]["bad"] else 0) for k, i in W.items(p)])
    start = np.zeros(n_mp + 1, np.int32)
    start[1:] = np.cumsum([len(r) for r in recs])
    obs = np.zeros(int(start[-1]), OBSERVATION_DTYPE)
    for j, r in enumerate([r for rr in recs for r in rr]):
        obs[j] = r
    view = dict(mp=mp, obs_start=start, obs=obs, kf=kf, kf_mp=np.asarray(rows, np.int32).reshape(-1), kf_by_order=np.asarray(W.order, np.int32))
    kfs = dict(ckf=ckf, feat=np.asarray(feat, np.uint8).reshape(-1), ref=ref, center=center,
               kf_desc=np.ascontiguousarray(np.concatenate(descs)) if descs else np.zeros((0, 32), np.uint8), mp_desc=mp_desc,
               mp_nobs=np.array([m["nObs"] for m in W.mps], np.int32), found=np.array([m["found"] for m in W.mps], np.int32),
               visible=np.array([m["visible"] for m in W.mps], np.int32),
               first_kf_id=np.array([m["first"] & 0xFFFFFFFF for m in W.mps], np.uint32).view(np.int32))
    return view, kfs


RECORDS = ("mp", "obs", "kf", "ckf", "ref", "center")


def rec_dev(a, backend):
    """to_dev, also for a record array without records (n_mp == 0)"""
    return to_dev(a, backend) if a.size or backend == "emu" else to_dev_plain(np.zeros((0, a.dtype.itemsize), np.uint8), backend)


def upload(view, kfs, backend):
    dev = lambda d: {k: (rec_dev(v, backend) if k in RECORDS else to_dev_plain(v, backend)) for k, v in d.items()}   # noqa: E731
    return dev(view), dev(kfs)


def host(a, dtype=None):
    a = to_host(a)
    return a if dtype is None or a.dtype.names else np.ascontiguousarray(a).view(dtype).reshape(-1)


def recent_arrays(recent, cap, backend):
    r = np.full(cap, -7, np.int32)
    r[:len(recent)] = recent
    return to_dev_plain(r, backend), to_dev_plain(np.array([len(recent)], np.int32), backend)


def rows_of(start, obs, p):
    return [(int(o["kf"]), int(o["desc_row"]), int(o["flags"])) for o in obs[start[p]:start[p + 1]]]


def compare_map(W, view_h, kfs_h, dv, dk, out, use_nobs, live_only=True):
    """the map as the device holds it after a call that fitted, against the restated world W"""
    want_v, want_k = flatten(W)
    start, obs = host(out["obs_start"]), host(out["obs"], OBSERVATION_DTYPE)
    assert start.tolist() == want_v["obs_start"].tolist()
    n = int(start[-1])
    assert obs[:n].tolist() == want_v["obs"].tolist()
    mp = host(dv["mp"], MAP_POINT_DTYPE)
    assert (mp["flags"] & (MP_VALID | MP_BAD)).tolist() == (want_v["mp"]["flags"] & (MP_VALID | MP_BAD)).tolist()
    assert host(dv["kf_mp"]).tolist() == want_v["kf_mp"].tolist()
    if use_nobs:
        assert host(dk["mp_nobs"]).tolist() == want_k["mp_nobs"].tolist()
    for p, m in enumerate(W.mps):
        if m["valid"] and not m["bad"]:
            for name in ("normal", "min_distance", "max_distance", "pos"):
                assert mp[p][name].tobytes() == want_v["mp"][p][name].tobytes(), (p, name)
            assert host(dk["mp_desc"])[p].tobytes() == m["desc"].tobytes(), p


def run_process(L, backend, W, cur, recent=(), cap_recent=None, cap_obs_out=None, use_nobs=True, csr=None, kf_mp_raw=None, cap_feat=None,
                variant=None, restated=True):
    """the call on the flattened world against the restatement -> (Result, out, result words)"""
    n_feat = len(W.kfs[cur]["mp"]) if 0 <= cur < len(W.kfs) and W.kfs[cur] is not None else 0
    cap_feat = cap_feat or max(n_feat, 1)
    cap_recent = cap_recent or max(len(recent) + n_feat, 1)
    n_obs = sum(len(m["obs"]) for m in W.mps)
    cap_obs_out = n_obs + n_feat if cap_obs_out is None else cap_obs_out
    view, kfs = flatten(W, csr, kf_mp_raw)
    if not use_nobs:
        del kfs["mp_nobs"]
    dv, dk = upload(view, kfs, backend)
    rec, n_rec = recent_arrays(recent, cap_recent, backend)
    nk = NewKeyFrame(SF, cap_recent, lib=L)
    out = nk.ProcessNewKeyFrame(dv, dk, cur, cap_feat, cap_obs_out, rec, n_rec)
    res = host(out["result"])
    if not restated:
        return None, (dv, dk, out), res
    R = restate_process(W, cur, list(recent), cap_recent, cap_obs_out, use_nobs, variant)
    code = host(out["code"])
    assert code[:n_feat].tolist() == R.code and not code[n_feat:].any()
    assert res[NEWKF_R_FLAGS] == R.flags, (res[NEWKF_R_FLAGS], R.flags)
    assert (res[NEWKF_R_N_ADDED], res[NEWKF_R_N_PUSHED], res[NEWKF_R_N_PUSH_REQUIRED], res[NEWKF_R_N_OBS]) == \
        (R.n_added, R.n_pushed, R.n_push_required, R.n_obs)
    assert int(host(n_rec)[0]) == len(R.recent) and host(rec)[:len(R.recent)].tolist() == R.recent
    assert (host(rec)[len(R.recent):] == -7).all()
    if R.sel is not None:
        assert host(out["sel"]).tolist() == R.sel + [-1] * (cap_feat - len(R.sel))
        compare_map(R.W, view, kfs, dv, dk, out, use_nobs)
        mp = host(dv["mp"], MAP_POINT_DTYPE)
        for p in R.sel:
            assert bool(mp[p]["flags"] & MP_HAS_OBS) == (R.W.mps[p]["nObs"] > 0)
    else:                                                       # the overflow: the map stays as given
        assert host(dv["mp"], MAP_POINT_DTYPE).tobytes() == view["mp"].tobytes()
        assert host(dk["mp_desc"]).tobytes() == kfs["mp_desc"].tobytes()
        if use_nobs:
            assert host(dk["mp_nobs"]).tolist() == kfs["mp_nobs"].tolist()
    return R, (dv, dk, out), res


def run_cull(L, backend, W, cur, recent, cap_recent=None, cap_obs_out=None, mono=False, use_nobs=True, csr=None, variant=None, restated=True):
    cap_recent = cap_recent or max(len(recent), 1)
    n_obs = sum(len(m["obs"]) for m in W.mps)
    cap_obs_out = n_obs if cap_obs_out is None else cap_obs_out
    view, kfs = flatten(W, csr)
    if not use_nobs:
        del kfs["mp_nobs"]
    dv, dk = upload(view, kfs, backend)
    rec, n_rec = recent_arrays(recent, cap_recent, backend)
    nk = NewKeyFrame(SF, cap_recent, lib=L)
    out = nk.MapPointCulling(dv, dk, cur, rec, n_rec, cap_obs_out, bMonocular=mono)
    res = host(out["result"])
    if not restated:
        return None, (dv, dk, out), res
    R = restate_cull(W, cur, list(recent), cap_obs_out, mono, use_nobs, variant)
    code = host(out["code"])
    assert code[:len(recent)].tolist() == R.code and not code[len(recent):].any()
    assert res[NEWKF_R_FLAGS] == R.flags and res[NEWKF_R_N_OBS] == R.n_obs and res[NEWKF_R_N_PUSH_REQUIRED] == len(recent)
    assert host(rec)[:len(recent)].tolist() == list(recent) and int(host(n_rec)[0]) == len(recent)   # the input list is not touched
    if R.flags & NEWKF_OBS_OVERFLOW:
        assert (res[NEWKF_R_N_ADDED], res[NEWKF_R_N_PUSHED]) == (0, 0)
        assert host(dv["mp"], MAP_POINT_DTYPE).tobytes() == view["mp"].tobytes() and host(dv["kf_mp"]).tolist() == view["kf_mp"].tolist()
        return R, (dv, dk, out), res
    assert (res[NEWKF_R_N_ADDED], res[NEWKF_R_N_PUSHED]) == (len(R.culled), len(R.recent))
    assert int(host(out["n_recent"])[0]) == len(R.recent) and host(out["recent"])[:len(R.recent)].tolist() == R.recent
    assert int(host(out["n_culled"])[0]) == len(R.culled)
    assert host(out["culled"]).tolist() == R.culled + [-1] * (cap_recent - len(R.culled))
    compare_map(R.W, view, kfs, dv, dk, out, use_nobs)
    return R, (dv, dk, out), res


# ------------------------------------------------------------------------------------------------ orbm_process_new_keyframe, constructed
def small_world(order=None, cur_stereo=(False, True, False, False)):
    """three old key frames 0..2 and the new one, 3, whose features hold the points 0..3; the points have records of the old ones"""
    kfs = [KF([0, 1, 2, 3], center=(0.1 * k, 0, 0)) for k in range(3)] + [KF([0, 1, 2, 3], stereo=cur_stereo, center=(0.5, 0, 0))]
    mps = [MP((0.3 * p, 0.1, 4.0 + p), obs={k: p for k in range(3)}) for p in range(4)]
    return World(kfs, mps, order)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("use_nobs", [True, False])
def test_add_mono_and_stereo(lib, backend, use_nobs):
    """+1 on a mono feature and +2 on a stereo one, from the array (which has drifted from the records) and from the record sum"""
    W = small_world()
    for m in W.mps:
        m["nObs"] += 5
    R, _, _ = run_process(lib, backend, W, 3, use_nobs=use_nobs)
    assert R.code == [NEWKF_CODE_ADDED] * 4
    base = 8 if use_nobs else 3
    assert [m["nObs"] for m in R.W.mps] == [base + 1, base + 2, base + 1, base + 1]


@pytest.mark.parametrize("backend", BACKENDS)
def test_exits_and_duplicates(lib, backend):
    """a point already in the key frame (pushed, no record added); one point in two features without a record (the first adds, the second
    is pushed); one point in two features with a record (pushed twice); a bad point and a null entry"""
    kfs = [KF([0, 1, 2, 3, 4]), KF([0, 1, 2, 3, 4]), KF([0, 1, None, 1, 2, 3, 2, 4], stereo=[False, False, False, True, False, False, False, False])]
    mps = [MP(obs={0: 0, 1: 0, 2: 0}), MP(obs={0: 1, 1: 1}), MP(obs={0: 2, 2: 4}), MP(obs={0: 3}, bad=True), MP(obs={1: 4})]
    W = World(kfs, mps)
    R, _, res = run_process(lib, backend, W, 2, recent=[4])
    assert R.code == [NEWKF_CODE_PUSHED, NEWKF_CODE_ADDED, NEWKF_CODE_NONE, NEWKF_CODE_PUSHED_DUP, NEWKF_CODE_PUSHED, NEWKF_CODE_BAD_POINT,
                      NEWKF_CODE_PUSHED, NEWKF_CODE_ADDED]
    assert R.recent == [4, 0, 1, 2, 2] and R.sel == [1, 4]
    assert R.W.mps[1]["obs"][2] == 1 and R.W.mps[1]["nObs"] == 3    # the FIRST feature's record and its (mono) weight


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("where", ["front", "middle", "end"])
def test_insert_position_under_a_pointer_order(lib, backend, where):
    """the new record enters at the key frame's rank, under a pointer order that is not the identity; appending it is the wrong variant"""
    order = {"front": [3, 2, 0, 1], "middle": [2, 3, 1, 0], "end": [1, 0, 2, 3]}[where]
    W = small_world(order)
    R, (dv, dk, out), _ = run_process(lib, backend, W, 3)
    rows = [k for k, _ in R.W.items(0)]
    assert rows.index(3) == {"front": 0, "middle": 1, "end": 3}[where]
    start, obs = host(out["obs_start"]), host(out["obs"], OBSERVATION_DTYPE)
    assert [r[0] for r in rows_of(start, obs, 0)] == rows
    wrong = restate_process(W, 3, [], 8, 99, variant="append_order")
    assert (where == "end") == ([k for k, _ in wrong.W.items(0, "append_order")] == rows)


def tie_world(where):
    """one point seen by 0, 1 and the new key frame 2 with three descriptors at mutual distance 2: every row median ties, so the first
    record in map order wins and the position of the new record decides the descriptor"""
    order = {"front": [2, 0, 1], "middle": [0, 2, 1], "end": [0, 1, 2]}[where]
    d = [desc_of(7, [1]), desc_of(7, [2]), desc_of(7, [3])]
    kfs = [KF([0], desc=[d[0]], center=(0, 0, 0)), KF([0], desc=[d[1]], center=(0.2, 0, 0)), KF([0], desc=[d[2]], center=(0.4, 0, 0))]
    return World(kfs, [MP(obs={0: 0, 1: 0}, desc=d[0])], order), d


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("where", ["front", "middle", "end"])
def test_insert_position_flips_a_descriptor_tie(lib, backend, where):
    W, d = tie_world(where)
    R, _, _ = run_process(lib, backend, W, 2)
    assert R.W.mps[0]["desc"].tobytes() == (d[2] if where == "front" else d[0]).tobytes()
    wrong = restate_process(W, 2, [], 8, 99, variant="append_order")
    assert (where == "front") == (wrong.W.mps[0]["desc"].tobytes() != R.W.mps[0]["desc"].tobytes())


@pytest.mark.parametrize("backend", BACKENDS)
def test_new_record_moves_the_median_choice(lib, backend):
    """two records a, b at distance 8 (a wins the tie); the new record c lies 1 from b and 9 from a: b's lower median drops to 1 and b wins"""
    a, b, c = desc_of(9), desc_of(9, range(8)), desc_of(9, range(9))
    kfs = [KF([0], desc=[a]), KF([0], desc=[b], center=(0.2, 0, 0)), KF([0], desc=[c], center=(0.4, 0, 0))]
    W = World(kfs, [MP(obs={0: 0, 1: 0}, desc=a)])
    R, _, _ = run_process(lib, backend, W, 2)
    assert R.W.mps[0]["desc"].tobytes() == b.tobytes()


@pytest.mark.parametrize("backend", BACKENDS)
def test_refresh_overflow_is_flagged(lib, backend):
    """a point of 1 024 usable records gains its 1 025th: the record is added, the refresh leaves the point alone and the call says so"""
    n = REFRESH_MAX_OBS
    kfs = [KF([0], center=(0.001 * k, 0, 0)) for k in range(n + 1)]
    W = World(kfs, [MP(obs={k: 0 for k in range(n)}, desc=desc_of(3), normal=(0.6, 0, 0.8))])
    R, _, res = run_process(lib, backend, W, n)
    assert res[NEWKF_R_FLAGS] == NEWKF_REFRESH_OVERFLOW and len(R.W.mps[0]["obs"]) == n + 1
    assert R.W.mps[0]["desc"].tobytes() == desc_of(3).tobytes() and tuple(R.W.mps[0]["normal"]) == (0.6, 0, 0.8)
    with pytest.raises(OrbHipError) as e:
        NewKeyFrame(SF, 4, lib=lib).check_flags(dict(result=np.array(res), caps=dict(cap_obs_out=0, cap_recent=4)))
    assert e.value.code == ORB_E_CAPACITY


@pytest.mark.parametrize("backend", BACKENDS)
def test_capacities_full_and_one_over(lib, backend):
    kfs = [KF([0, 1, 2, 3]), KF([0, 0, 1, 1, 2, 3])]
    W = World(kfs, [MP(obs={0: 0, 1: 0}), MP(obs={0: 1, 1: 2}), MP(obs={0: 2}), MP(obs={0: 3})])
    # four pushes (0, 0, 1, 1) behind two entries: a list of six is full, of five one over
    R, _, _ = run_process(lib, backend, W, 1, recent=[3, 2], cap_recent=6)
    assert R.flags == 0 and R.recent == [3, 2, 0, 0, 1, 1]
    R, _, _ = run_process(lib, backend, W, 1, recent=[3, 2], cap_recent=5)
    assert R.flags == NEWKF_RECENT_OVERFLOW and R.recent == [3, 2, 0, 0, 1] and (R.n_pushed, R.n_push_required) == (3, 4)
    # six records and two new ones: eight fit, seven do not, and then nothing is written but the codes and the result
    R, _, _ = run_process(lib, backend, W, 1, recent=[3], cap_obs_out=8)
    assert R.flags == 0 and R.n_obs == 8
    R, (dv, dk, out), res = run_process(lib, backend, W, 1, recent=[3], cap_obs_out=7)
    assert R.flags == NEWKF_OBS_OVERFLOW and R.recent == [3] and res[NEWKF_R_N_OBS] == 8
    with pytest.raises(OrbHipError) as e:
        NewKeyFrame(SF, 4, lib=lib).check_flags(out)
    assert e.value.code == ORB_E_CAPACITY


@pytest.mark.parametrize("backend", BACKENDS)
def test_bad_indices_are_flagged_and_absent(lib, backend):
    W = small_world()
    W.mps.append(MP(valid=False, nObs=0))                                             # an empty slot, 4
    # a d_kf_mp entry out of range, one below -1, and one that names the empty slot
    _, (dv, dk, out), res = run_process(lib, backend, W, 3, kf_mp_raw={(3, 0): 99, (3, 1): -2, (3, 2): 4}, restated=False)
    assert res[NEWKF_R_FLAGS] == NEWKF_BAD_INDEX
    assert host(out["code"]).tolist() == [NEWKF_CODE_BAD_INDEX] * 3 + [NEWKF_CODE_ADDED]
    assert host(out["sel"]).tolist() == [3, -1, -1, -1] and res[NEWKF_R_N_ADDED] == 1
    with pytest.raises(OrbHipError) as e:
        NewKeyFrame(SF, 4, lib=lib).check_flags(out)
    assert e.value.code == ORB_E_INVALID
    # a record whose key frame is out of range / an empty slot / whose row is outside its key frame: absent (so not "in the key frame")
    W2 = small_world()
    W2.kfs.append(None)                                                       # an empty key-frame slot, 4
    W2.order.append(4)
    for rec in [(9, 0, 0), (4, 0, 0), (3, 7, 0), (-1, 0, 0)]:
        _, (dv, dk, out), res = run_process(lib, backend, W2, 3, csr={0: [(0, 0, 0), rec]}, restated=False)
        assert res[NEWKF_R_FLAGS] == NEWKF_BAD_INDEX, rec
        assert host(out["code"]).tolist() == [NEWKF_CODE_ADDED] * 4
        start, obs = host(out["obs_start"]), host(out["obs"], OBSERVATION_DTYPE)
        assert [r[0] for r in rows_of(start, obs, 0)] == [0, rec[0], 3]       # the rows as they lie, the new record at the end
        assert host(dk["mp_nobs"])[0] == 3 + 1
    # the record sum leaves the absent record out
    _, (dv, dk, out), res = run_process(lib, backend, W2, 3, csr={0: [(0, 0, 0), (9, 0, 0)]}, use_nobs=False, restated=False)
    assert host(dv["mp"], MAP_POINT_DTYPE)[0]["flags"] & MP_HAS_OBS
    # a CSR range that leaves the slab: the point has no rows
    view, kfs = flatten(W)
    view["obs_start"][2] = 99
    dv, dk = upload(view, kfs, backend)
    rec, n_rec = recent_arrays([], 8, backend)
    out = NewKeyFrame(SF, 8, lib=lib).ProcessNewKeyFrame(dv, dk, 3, 4, 64, rec, n_rec)
    assert host(out["result"])[NEWKF_R_FLAGS] & NEWKF_BAD_INDEX
    # n_feat above cap_feat, desc_row0 outside the slab, a key frame that is not there: no feature is visited
    for breakage in ("cap_feat", "desc_row0", "absent", "range"):
        view, kfs = flatten(W)
        cur, cap_feat = 3, 4
        if breakage == "cap_feat":
            cap_feat = 3
        elif breakage == "desc_row0":
            kfs["ckf"][3]["desc_row0"] = len(kfs["kf_desc"]) - 3
        elif breakage == "absent":
            view["kf"][3]["flags"] = 0
        else:
            cur = 17
        dv, dk = upload(view, kfs, backend)
        rec, n_rec = recent_arrays([1], 8, backend)
        out = NewKeyFrame(SF, 8, lib=lib).ProcessNewKeyFrame(dv, dk, cur, cap_feat, 64, rec, n_rec)
        res = host(out["result"])
        assert res[NEWKF_R_FLAGS] == NEWKF_BAD_INDEX and not host(out["code"]).any(), breakage
        assert (res[NEWKF_R_N_ADDED], res[NEWKF_R_N_PUSHED], res[NEWKF_R_N_OBS]) == (0, 0, 12)
        assert host(out["obs"], OBSERVATION_DTYPE)[:12].tolist() == view["obs"].tolist() and int(host(n_rec)[0]) == 1
    # a cursor outside the list
    view, kfs = flatten(W)
    dv, dk = upload(view, kfs, backend)
    rec, n_rec = recent_arrays([], 8, backend)
    n_rec[0] = 9
    out = NewKeyFrame(SF, 8, lib=lib).ProcessNewKeyFrame(dv, dk, 3, 4, 64, rec, n_rec)
    assert host(out["result"])[NEWKF_R_FLAGS] == NEWKF_BAD_INDEX and int(host(n_rec)[0]) == 8


@pytest.mark.parametrize("backend", BACKENDS)
def test_rig_record_and_unsorted_rows(lib, backend):
    W = small_world([2, 0, 3, 1])
    # the rig record of the current key frame is absent: the point is not "in the key frame" and gains a record
    _, (dv, dk, out), res = run_process(lib, backend, W, 3, csr={1: [(2, 1, 0), (3, 1, OBS_RIGHT)]}, restated=False)
    assert res[NEWKF_R_FLAGS] == NEWKF_UNSUPPORTED and host(out["code"]).tolist() == [NEWKF_CODE_ADDED] * 4
    # rows that are not in ascending rank (rank order is 2, 0, 3, 1) are copied as they lie; the record goes before the first greater rank
    _, (dv, dk, out), res = run_process(lib, backend, W, 3, csr={1: [(1, 1, 0), (2, 1, 0), (0, 1, 0)]}, restated=False)
    assert res[NEWKF_R_FLAGS] == NEWKF_UNSORTED
    start, obs = host(out["obs_start"]), host(out["obs"], OBSERVATION_DTYPE)
    assert [r[0] for r in rows_of(start, obs, 1)] == [3, 1, 2, 0]
    NewKeyFrame(SF, 4, lib=lib).check_flags(out)                              # not an error


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n_feat", [WG - 1, WG, WG + 1])
def test_chunk_edges(lib, backend, n_feat):
    """features across the chunk of 256, points across several blocks of the CSR scan (n_mp above 256 and no multiple of it)"""
    rng = np.random.default_rng(n_feat)
    n_mp = 2 * WG + 77
    mp_of = rng.integers(0, n_mp, n_feat).tolist()
    for i in range(0, n_feat, 9):
        mp_of[i] = None
    kfs = [KF(list(range(n_mp))), KF(mp_of, stereo=(rng.random(n_feat) < 0.5).tolist(), center=(0.3, 0, 0))]
    mps = [MP(rng.normal(0, 1, 3) + [0, 0, 5], obs={0: p, 1: mp_of.index(p)} if p in mp_of and p % 3 == 0 else {0: p}, bad=p % 11 == 0)
           for p in range(n_mp)]
    R, _, _ = run_process(lib, backend, World(kfs, mps, [1, 0]), 1, recent=[5, 6])
    assert {NEWKF_CODE_ADDED, NEWKF_CODE_PUSHED, NEWKF_CODE_PUSHED_DUP, NEWKF_CODE_BAD_POINT, NEWKF_CODE_NONE} <= set(R.code)


@pytest.mark.parametrize("backend", BACKENDS)
def test_empty_shapes(lib, backend):
    # an empty key frame
    W = World([KF([0]), KF([])], [MP(obs={0: 0})])
    R, _, res = run_process(lib, backend, W, 1, recent=[0])
    assert (res[NEWKF_R_N_ADDED], res[NEWKF_R_N_OBS]) == (0, 1) and R.recent == [0]
    # no points at all
    W = World([KF([None, None])], [])
    R, (dv, dk, out), res = run_process(lib, backend, W, 0)
    assert R.code == [NEWKF_CODE_NONE] * 2 and host(out["obs_start"]).tolist() == [0]
    R, _, res = run_cull(lib, backend, W, 0, [])
    assert res.tolist() == [0] * 8
    # an empty list
    R, _, res = run_cull(lib, backend, small_world(), 3, [])
    assert res[NEWKF_R_N_OBS] == 12


# ------------------------------------------------------------------------------------------------ orbm_cull_map_points, constructed
def cull_world(points, cur_id=110, n_old=3):
    """points: dicts(found, visible, first, n (records, mono), bad, nObs); key frame n_old is the current one with id cur_id"""
    n = len(points)
    kfs = [KF(list(range(n))) for _ in range(n_old)] + [KF([None] * n, id=cur_id)]
    mps = []
    for p, d in enumerate(points):
        d = dict(d)
        nrec = d.pop("n", 4)
        mps.append(MP(obs={k: p for k in range(min(nrec, n_old))}, **d))
        for k in range(min(nrec, n_old), n_old):
            kfs[k]["mp"][p] = None
    return World(kfs, mps)


@pytest.mark.parametrize("backend", BACKENDS)
def test_cull_each_exit_and_the_order_of_the_chain(lib, backend):
    pts = [dict(bad=True), dict(found=1, visible=5), dict(first=108, n=3), dict(first=107, nObs=9), dict(first=109),
           # several tests at once: the first in the reference's order wins
           dict(bad=True, found=0, visible=9, first=100, n=1), dict(found=0, visible=9, first=100, n=1), dict(first=100, n=2)]
    W = cull_world(pts)
    R, _, _ = run_cull(lib, backend, W, 3, list(range(8)))
    assert R.code == [MPCULL_CODE_ERASED_BAD, MPCULL_CODE_CULLED_RATIO, MPCULL_CODE_CULLED_OBS, MPCULL_CODE_RETIRED, MPCULL_CODE_KEPT,
                      MPCULL_CODE_ERASED_BAD, MPCULL_CODE_CULLED_RATIO, MPCULL_CODE_CULLED_OBS]
    assert R.culled == [1, 2, 6, 7] and R.recent == [4]
    for k in range(3):
        assert R.W.kfs[k]["mp"][1] is None and R.W.kfs[k]["mp"][2] is None
    assert R.W.mps[1]["nObs"] == 3 and R.W.mps[1]["found"] == 1                # nObs, found and visible stay


def quotient_pair():
    """(found, visible) above 2^24 whose rounded float quotient is not below 0.25 although the exact rational is"""
    for visible in range(2 ** 26 + 1, 2 ** 26 + 64):
        for found in range(2 ** 24 + 1, 2 ** 24 + 16):
            if 4 * found < visible and not f32(found) / f32(visible) < f32(0.25):
                return found, visible
    raise AssertionError("no such pair")


@pytest.mark.parametrize("backend", BACKENDS)
def test_cull_found_ratio(lib, backend):
    found, visible = quotient_pair()
    assert found > 2 ** 24 and visible > 2 ** 24
    pts = [dict(found=25, visible=100), dict(found=24, visible=100), dict(found=26, visible=100), dict(found=found, visible=visible),
           dict(found=0, visible=0), dict(found=3, visible=0), dict(found=-1, visible=0)]
    W = cull_world([dict(d, first=110) for d in pts])
    R, _, _ = run_cull(lib, backend, W, 3, list(range(7)))
    K, C = MPCULL_CODE_KEPT, MPCULL_CODE_CULLED_RATIO
    assert R.code == [K, C, K, K, K, K, C]                                     # 0/0 = NaN and 3/0 = inf are not below; -1/0 = -inf is
    wrong = restate_cull(W, 3, list(range(7)), 99, variant="int_ratio")
    assert wrong.code[3] == C and wrong.code != R.code


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("use_nobs", [True, False])
def test_cull_observation_threshold_and_id_difference(lib, backend, mono, use_nobs):
    th = 2 if mono else 3
    # nObs at nThObs and one above, at difference 2; from the array the records say something else
    pts = [dict(first=108, n=th, nObs=th if use_nobs else 7), dict(first=108, n=th + 1, nObs=th + 1 if use_nobs else 0),
           dict(first=109, n=1), dict(first=108, n=4), dict(first=107, n=4), dict(first=111, n=1), dict(first=2 ** 32 - 5, n=4)]
    W = cull_world(pts, n_old=4)
    R, _, _ = run_cull(lib, backend, W, 4, list(range(7)), mono=mono, use_nobs=use_nobs)
    assert R.code == [MPCULL_CODE_CULLED_OBS, MPCULL_CODE_KEPT, MPCULL_CODE_KEPT, MPCULL_CODE_KEPT, MPCULL_CODE_RETIRED, MPCULL_CODE_KEPT,
                      MPCULL_CODE_RETIRED]                                     # 110 - (int)(2^32 - 5) = 115


@pytest.mark.parametrize("backend", BACKENDS)
def test_cull_duplicates(lib, backend):
    """the first occurrence decides: culled -> the later ones find it bad; kept or retired -> every occurrence takes the same exit"""
    W = cull_world([dict(found=0, visible=4), dict(first=109), dict(first=100, nObs=9), dict(first=100, n=1)])
    R, _, _ = run_cull(lib, backend, W, 3, [0, 1, 2, 0, 3, 1, 2, 3, 0])
    assert R.code == [MPCULL_CODE_CULLED_RATIO, MPCULL_CODE_KEPT, MPCULL_CODE_RETIRED, MPCULL_CODE_ERASED_BAD, MPCULL_CODE_CULLED_OBS,
                      MPCULL_CODE_KEPT, MPCULL_CODE_RETIRED, MPCULL_CODE_ERASED_BAD, MPCULL_CODE_ERASED_BAD]
    assert R.culled == [0, 3] and R.recent == [1, 1]


@pytest.mark.parametrize("backend", BACKENDS)
def test_cull_erases_the_feature_slot_whatever_it_holds(lib, backend):
    """two culled points whose records name the same feature slot, and a culled point whose slot holds another point"""
    kfs = [KF([2, 2, 1]), KF([None] * 3, id=110)]
    mps = [MP(obs={0: 0}, found=0, visible=9), MP(obs={0: 0}, found=0, visible=9), MP(obs={0: 1}, first=110)]
    W = World(kfs, mps)
    R, (dv, dk, out), _ = run_cull(lib, backend, W, 1, [0, 1, 2])
    assert R.culled == [0, 1] and R.W.kfs[0]["mp"] == [None, 2, 1] and host(dv["kf_mp"])[:3].tolist() == [-1, 2, 1]


@pytest.mark.parametrize("backend", BACKENDS)
def test_cull_capacity_and_bad_indices(lib, backend):
    W = cull_world([dict(found=0, visible=9), dict(first=110), dict(first=110)])
    R, _, _ = run_cull(lib, backend, W, 3, [0, 1], cap_obs_out=6)               # nine records, three leave: six fit
    assert R.flags == 0
    R, (dv, dk, out), _ = run_cull(lib, backend, W, 3, [0, 1], cap_obs_out=5)
    assert R.flags == NEWKF_OBS_OVERFLOW and R.code[0] == MPCULL_CODE_CULLED_RATIO
    # list entries that cannot be read are dropped and flagged
    W.mps.append(MP(valid=False, nObs=0))
    _, (dv, dk, out), res = run_cull(lib, backend, W, 3, [1, -1, 3, 77, 2], restated=False)
    assert res[NEWKF_R_FLAGS] == NEWKF_BAD_INDEX
    assert host(out["code"]).tolist() == [MPCULL_CODE_KEPT] + [MPCULL_CODE_BAD_INDEX] * 3 + [MPCULL_CODE_KEPT]
    assert host(out["recent"])[:2].tolist() == [1, 2] and int(host(out["n_recent"])[0]) == 2
    # records that cannot be read: no slot is erased through them, the sum leaves them out; a rig record likewise
    for rec, flag in [((9, 0, 0), NEWKF_BAD_INDEX), ((1, 5, 0), NEWKF_BAD_INDEX), ((1, 0, OBS_RIGHT), NEWKF_UNSUPPORTED)]:
        _, (dv, dk, out), res = run_cull(lib, backend, W, 3, [0], csr={0: [(0, 0, 0), rec]}, restated=False)
        assert res[NEWKF_R_FLAGS] == flag and host(out["culled"]).tolist() == [0]
        assert host(dv["kf_mp"])[[0, 3]].tolist() == [-1, 0]
    # a current key frame that cannot be read: nothing is visited
    _, (dv, dk, out), res = run_cull(lib, backend, W, 9, [0, 1], restated=False)
    assert res[NEWKF_R_FLAGS] == NEWKF_BAD_INDEX and not host(out["code"]).any() and int(host(out["n_recent"])[0]) == 0
    # a CSR range that leaves the slab
    view, kfs = flatten(W)
    view["obs_start"][1] = -4
    dv, dk = upload(view, kfs, backend)
    rec, n_rec = recent_arrays([0], 4, backend)
    out = NewKeyFrame(SF, 4, lib=lib).MapPointCulling(dv, dk, 3, rec, n_rec, 16)
    assert host(out["result"])[NEWKF_R_FLAGS] & NEWKF_BAD_INDEX


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n_list", [WG - 1, WG, WG + 1])
def test_cull_chunk_edges(lib, backend, n_list):
    rng = np.random.default_rng(n_list)
    n_mp = WG + 91
    pts = [dict(found=int(rng.integers(0, 8)), visible=int(rng.integers(0, 12)), first=int(rng.integers(105, 112)), n=int(rng.integers(1, 5)),
                bad=bool(rng.random() < 0.1)) for _ in range(n_mp)]
    W = cull_world(pts, n_old=4)
    R, _, _ = run_cull(lib, backend, W, 4, rng.integers(0, n_mp, n_list).tolist())
    assert set(R.code) == {MPCULL_CODE_ERASED_BAD, MPCULL_CODE_CULLED_RATIO, MPCULL_CODE_CULLED_OBS, MPCULL_CODE_RETIRED, MPCULL_CODE_KEPT}


# ------------------------------------------------------------------------------------------------ more than 256 blocks of points
BIG_N = 256 * WG + 300   # 258 blocks of 256 point slots: the one-workgroup scan of the block totals (csrc/obs_csr.inc) takes a second chunk
BIG_PTS = [3, 4, 300, 301, 20000, 65535, 65536, 65537, 65800, 65801, BIG_N - 1]   # the points with records, on both sides of block 256
BIG_CUR = [3, 300, 65535, 65536, 65800, BIG_N - 1, None, 4, 65537]                # the new key frame's features; 4 and 65537 have its record


def big_world():
    """BIG_N point slots, nearly all empty (one dict stands in every empty slot: nothing touches it).  Three old key frames 0..2 hold the
    points BIG_PTS, the new one, 3, holds BIG_CUR.  The slots 10 and 65700 are valid points without records.  The points 4 and 65801 are
    found too seldom (MapPointCulling culls them), the others were made by the new key frame (it keeps them)"""
    kfs = [KF(BIG_PTS, center=(0.1 * k, 0, 0)) for k in range(3)] + [KF(BIG_CUR, stereo=[i % 2 == 1 for i in range(len(BIG_CUR))], center=(0.5, 0, 0))]
    mps = [MP(valid=False)] * BIG_N
    for j, p in enumerate(BIG_PTS):
        obs = {k: j for k in range(3)}
        if p in (4, 65537):
            obs[3] = BIG_CUR.index(p)
        mps[p] = MP((0.02 * j, 0.1, 4.0 + 0.1 * j), obs=obs, first=103, found=0 if p in (4, 65801) else 1, visible=1)
    mps[10], mps[65700] = MP(first=103), MP(first=103)
    return World(kfs, mps, [2, 0, 3, 1])


@pytest.mark.parametrize("backend", BACKENDS)
def test_process_scans_more_than_256_blocks(lib, backend):
    """the offsets of the second chunk of the block scan continue the first's: records are inserted in blocks on both sides of block 256, and
    the rows of the points behind them move"""
    R, _, _ = run_process(lib, backend, big_world(), 3)
    assert R.sel == BIG_CUR[:6] and any(p < 256 * WG for p in R.sel) and any(p >= 256 * WG for p in R.sel)
    assert R.recent == [4, 65537] and R.n_obs == 3 * len(BIG_PTS) + 2 + 6


@pytest.mark.parametrize("backend", BACKENDS)
def test_cull_scans_more_than_256_blocks(lib, backend):
    """the same map: a point culled and a point kept on each side of block 256"""
    R, _, _ = run_cull(lib, backend, big_world(), 3, [4, 3, 65801, 65536, 65535, BIG_N - 1])
    assert R.culled == [4, 65801] and R.recent == [3, 65536, 65535, BIG_N - 1]
    assert any(p < 256 * WG for p in R.culled) and any(p >= 256 * WG for p in R.culled)
    assert any(p < 256 * WG for p in R.recent) and any(p >= 256 * WG for p in R.recent)
    assert R.n_obs == 3 * len(BIG_PTS) + 2 - 4 - 3


# ------------------------------------------------------------------------------------------------ random worlds
def random_world(rng):
    n_kf = int(rng.integers(2, 13))
    n_mp = int(rng.integers(1, 60))
    kfs = []
    for k in range(n_kf):
        nf = int(rng.integers(0, 41))
        mp = [int(rng.integers(0, n_mp)) if rng.random() < 0.7 else None for _ in range(nf)]
        kfs.append(KF(mp, stereo=(rng.random(nf) < 0.4).tolist(), center=rng.normal(0, 0.5, 3), id=int(rng.integers(100, 106)),
                      bad=bool(rng.random() < 0.1), desc=rng.integers(0, 256, (nf, 32), dtype=np.uint8) if nf else None))
    cur = int(rng.integers(0, n_kf))
    kfs[cur]["bad"] = False
    mps = []
    for p in range(n_mp):
        obs = {}
        for k in range(n_kf):
            held = [i for i, q in enumerate(kfs[k]["mp"]) if q == p]
            if held and rng.random() < (0.3 if k == cur else 0.8):
                obs[k] = held[int(rng.integers(0, len(held)))]
        mps.append(MP(rng.normal(0, 1, 3) + [0, 0, 6], obs=obs, bad=bool(rng.random() < 0.1), found=int(rng.integers(0, 6)),
                      visible=int(rng.integers(0, 9)), first=int(rng.integers(98, 108)), ref_kf=int(rng.integers(0, n_kf)),
                      level=int(rng.integers(0, NLEVELS)), nObs=None if rng.random() < 0.7 else int(rng.integers(0, 7))))
    return World(kfs, mps, rng.permutation(n_kf).tolist()), cur


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("block", range(4))
def test_random_worlds(lib, backend, block):
    rng = np.random.default_rng(4100 + block)
    for _ in range(60):
        W, cur = random_world(rng)
        recent = rng.integers(0, len(W.mps), int(rng.integers(0, 30))).tolist()
        use_nobs = bool(rng.random() < 0.5)
        run_process(lib, backend, W, cur, recent=recent, use_nobs=use_nobs, cap_recent=len(recent) + int(rng.integers(1, 30)))
        run_cull(lib, backend, W, cur, recent, mono=bool(rng.random() < 0.5), use_nobs=use_nobs)


# ------------------------------------------------------------------------------------------------ the chain of LocalMapping::Run
def dev_set(a, idx, values):
    """entries of a device array, written where the array lies"""
    if isinstance(a, np.ndarray):
        a[idx] = values
    else:
        import torch
        a[torch.as_tensor(idx, device=a.device, dtype=torch.long)] = torch.as_tensor(values, device=a.device, dtype=a.dtype)


@pytest.mark.parametrize("backend", BACKENDS)
def test_chain_over_four_keyframes(lib, backend):
    """process -> cull -> orbm_append_new_map_points on the out-CSR -> push -> the next key frame, on device arrays alone: each call reads the
    CSR the call before it wrote.  Points pass through id differences 0 to 3; the map is compared with the restatement after every step."""
    NF, NEW, OLD, STEPS = 16, 3, 2, 4
    n_kf, n_mp0, cap_mp = OLD + STEPS, 8, 8 + NEW * STEPS
    # key frame OLD + s holds: the initial points (some without a record yet), then what the steps before it created
    kfs = [KF([p if p < n_mp0 else None for p in range(NF)], center=(0.1 * k, 0, 0), id=100 + k,
              stereo=[(k + i) % 3 == 0 for i in range(NF)], oct=[i % NLEVELS for i in range(NF)]) for k in range(n_kf)]
    mps = [MP((0.2 * p, 0.1, 5.0 + 0.1 * p), obs={0: p, 1: p}, found=1 + p % 3, visible=2 + p % 5, first=100 + p % 2, level=p % 3)
           for p in range(n_mp0)]
    mps[5]["bad"] = True
    mps += [MP(valid=False) for _ in range(cap_mp - n_mp0)]
    W = World(kfs, mps, [3, 0, 5, 1, 4, 2])
    recent, cursor = [0, 1, 2, 5], n_mp0
    cap_recent, cap_obs = 40, 160
    view, kk = flatten(W)
    view["obs"] = np.concatenate([view["obs"], np.zeros(cap_obs - len(view["obs"]), OBSERVATION_DTYPE)])
    # what the steps will create is known ahead: its per-point arrays can lie in place from the start (the slots are not VALID yet)
    for s in range(STEPS):
        for r in range(NEW):
            p = n_mp0 + NEW * s + r
            kk["found"][p], kk["visible"][p], kk["mp_nobs"][p] = 1 + r, 2 + r, 2
            kk["first_kf_id"][p] = 100 + OLD + s
            kk["mp_desc"][p] = desc_of(p)
    dv, dk = upload(view, kk, backend)
    other = dict(obs_start=to_dev_plain(np.zeros(cap_mp + 1, np.int32), backend), obs=to_dev(np.zeros(cap_obs, OBSERVATION_DTYPE), backend))
    rec, n_rec = recent_arrays(recent, cap_recent, backend)
    n_mp_dev = to_dev_plain(np.array([cursor], np.int32), backend)
    nk = NewKeyFrame(SF, cap_recent, lib=lib)
    kps1 = np.zeros((1, NF), KP_DTYPE)
    kps1["octave"] = [i % NLEVELS for i in range(NF)]
    d_kps1 = to_dev(kps1, backend)
    for s in range(STEPS):
        cur = OLD + s
        # -- ProcessNewKeyFrame: view (A) -> other (B)
        outP = dict(code=to_dev_plain(np.zeros(NF, np.uint8), backend), sel=to_dev_plain(np.zeros(NF, np.int32), backend), obs_start=other["obs_start"],
                    obs=other["obs"], result=to_dev_plain(np.zeros(8, np.int32), backend))
        nk.ProcessNewKeyFrame(dv, dk, cur, NF, cap_obs, rec, n_rec, out=outP)
        R = restate_process(W, cur, recent, cap_recent, cap_obs)
        assert host(outP["code"]).tolist() == R.code and host(outP["result"])[NEWKF_R_FLAGS] == 0
        W, recent = R.W, R.recent
        assert host(rec)[:int(host(n_rec)[0])].tolist() == recent
        # -- MapPointCulling: B -> A
        vB = dict(dv, obs_start=other["obs_start"], obs=other["obs"])
        outC = dict(code=to_dev_plain(np.zeros(cap_recent, np.uint8), backend), recent=to_dev_plain(np.zeros(cap_recent, np.int32), backend),
                    n_recent=to_dev_plain(np.zeros(1, np.int32), backend), culled=to_dev_plain(np.zeros(cap_recent, np.int32), backend),
                    n_culled=to_dev_plain(np.zeros(1, np.int32), backend), obs_start=dv["obs_start"], obs=dv["obs"],
                    result=to_dev_plain(np.zeros(8, np.int32), backend))
        nk.MapPointCulling(vB, dk, cur, rec, n_rec, cap_obs, out=outC)
        R = restate_cull(W, cur, recent, cap_obs)
        assert host(outC["code"])[:len(recent)].tolist() == R.code and host(outC["result"])[NEWKF_R_FLAGS] == 0
        assert host(outC["culled"])[:len(R.culled)].tolist() == R.culled
        W, recent = R.W, R.recent
        rec, n_rec = outC["recent"], outC["n_recent"]                          # the caller ping-pongs the list
        # -- CreateNewMapPoints' tail: NEW points between the current key frame and the one before it, appended to A behind the cursor
        prev = cur - 1
        new = np.zeros((1, NEW), NEW_POINT_DTYPE)
        pairs = np.zeros(1, NEWPT_PAIR_DTYPE)
        pairs["kf1"], pairs["kf2"], pairs["desc_row0_1"], pairs["desc_row0_2"] = cur, prev, cur * NF, prev * NF
        pairs["obs_kf2_first"] = int(W.rank[prev] < W.rank[cur])
        for r in range(NEW):
            i1, i2 = n_mp0 + r, 15 - r                                         # features of the two key frames that hold no point
            p = cursor + r
            new[0, r]["pos"], new[0, r]["idx1"], new[0, r]["idx2"] = (0.1 * p, -0.2, 6.0), i1, i2
            W.mps[p] = MP(new[0, r]["pos"], obs={cur: i1, prev: i2}, found=1 + r, visible=2 + r, first=100 + cur, ref_kf=cur, level=i1 % NLEVELS,
                          desc=desc_of(p), normal=(0, 0, 0), min_d=f32(0), max_d=f32(0), nObs=2)
            W.kfs[cur]["mp"][i1], W.kfs[prev]["mp"][i2] = p, p
            dev_set(dv["kf_mp"], [cur * NF + i1, prev * NF + i2], [p, p])       # pKF->AddMapPoint, where the table lies
            if s + 1 < STEPS and r < 2:                                        # the next key frame sees two of them, without a record yet
                W.kfs[cur + 1]["mp"][n_mp0 + NEW + r] = p
                dev_set(dv["kf_mp"], [(cur + 1) * NF + n_mp0 + NEW + r], [p])
        sel = to_dev_plain(np.zeros(NEW + 2, np.int32), backend)
        appended = to_dev_plain(np.zeros(2, np.int32), backend)
        d_new, d_nnew, d_pairs = to_dev(new, backend), to_dev_plain(np.array([NEW], np.int32), backend), to_dev(pairs, backend)
        rc = lib.orbm_append_new_map_points(ptr(d_new), ptr(d_nnew), NEW, ptr(d_pairs), 1, ptr(d_kps1), NF, ptr(n_mp_dev), ptr(dv["mp"]), cap_mp, cap_mp,
                                            ptr(dv["obs_start"]), ptr(dv["obs"]), cap_obs, ptr(dk["ref"]), ptr(sel), NEW + 2, ptr(appended), None)
        assert rc == 0 and host(appended).tolist() == [NEW, 0]
        cursor += NEW
        # -- mlpRecentAddedMapPoints.push_back
        outR = nk.PushRecent(sel, rec, n_rec)
        recent = recent + list(range(cursor - NEW, cursor))
        assert host(outR["result"]).tolist() == [0, 0, NEW, NEW, 0, 0, 0, 0]
        assert host(rec)[:int(host(n_rec)[0])].tolist() == recent
        # -- the map after the step
        want_v, want_k = flatten(W)
        n = int(want_v["obs_start"][cursor])
        assert host(dv["obs_start"])[:cursor + 1].tolist() == want_v["obs_start"][:cursor + 1].tolist()
        assert host(dv["obs"], OBSERVATION_DTYPE)[:n].tolist() == want_v["obs"].tolist()
        assert host(dv["kf_mp"]).tolist() == want_v["kf_mp"].tolist()
        mp = host(dv["mp"], MAP_POINT_DTYPE)
        assert (mp["flags"] & (MP_VALID | MP_BAD)).tolist() == (want_v["mp"]["flags"] & (MP_VALID | MP_BAD)).tolist()
        assert host(dk["mp_nobs"])[:cursor].tolist() == want_k["mp_nobs"][:cursor].tolist()
        for p in range(cursor):
            if not W.mps[p]["bad"]:
                assert mp[p]["normal"].tobytes() == want_v["mp"][p]["normal"].tobytes() and mp[p]["max_distance"] == want_v["mp"][p]["max_distance"], p
                assert host(dk["mp_desc"])[p].tobytes() == W.mps[p]["desc"].tobytes(), p
    firsts = {int32(100 + OLD + STEPS - 1) - m["first"] for m in W.mps if m["valid"]}
    assert {0, 1, 2, 3} <= firsts


# ------------------------------------------------------------------------------------------------ the argument checks
@pytest.mark.parametrize("backend", BACKENDS)
def test_argument_errors(lib, backend):
    W = small_world()
    view, kk = flatten(W)
    dv, dk = upload(view, kk, backend)
    nk = NewKeyFrame(SF, 8, lib=lib)
    rec, n_rec = recent_arrays([], 8, backend)
    out = nk.ProcessNewKeyFrame(dv, dk, 3, 4, 64, rec, n_rec)
    V = NewKeyFrame._view(dv)
    I = nk._in(V, dk, 4)

    def O(**kw):
        o = NewKfOut(ptr(dv["mp"]).value, ptr(dk["mp_nobs"]).value, ptr(dk["mp_desc"]).value, ptr(out["code"]).value, ptr(out["sel"]).value,
                     ptr(out["obs_start"]).value, ptr(out["obs"]).value, ptr(rec).value, ptr(n_rec).value, ptr(out["result"]).value, 4, 64, 8, 0)
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    work, ref = ptr(out["work"]), ctypes.byref
    call = lambda v=V, i=I, p=nk.params, o=None, w=work: lib.orbm_process_new_keyframe(ref(v), ref(i), 3, ref(p), ref(o or O()), w, None)   # noqa: E731
    assert call() == 0
    assert lib.orbm_process_new_keyframe(None, ref(I), 3, ref(nk.params), ref(O()), work, None) == ORB_E_INVALID
    assert lib.orbm_process_new_keyframe(ref(V), ref(I), 3, ref(nk.params), ref(O()), None, None) == ORB_E_INVALID
    assert call(w=ctypes.c_void_p(work.value + 4)) == ORB_E_INVALID
    for field in ("d_code", "d_sel", "d_obs_start_out", "d_obs_out", "d_recent", "d_n_recent", "d_result", "d_mp", "d_mp_desc"):
        assert call(o=O(**{field: None})) == ORB_E_INVALID, field
    assert call(o=O(d_mp_nobs=None)) == 0
    for field, v in (("cap_recent", 0), ("cap_obs_out", -1), ("n_desc_rows", -1), ("d_obs_start_out", V.d_obs_start), ("d_obs_out", V.d_obs),
                     ("d_mp_desc", ptr(dk["mp_desc"]).value + 8)):
        assert call(o=O(**{field: v})) == ORB_E_INVALID, field
    for field, v in (("cap_feat", 0), ("n_kf_desc_rows", -1), ("d_ckf", None), ("d_feat", None), ("d_ref", None), ("d_center", None),
                     ("d_kf_desc", None)):
        i2 = NewKfIn.from_buffer_copy(I)
        setattr(i2, field, v)
        assert call(i=i2) == ORB_E_INVALID, field
    for field, v in (("n_mp", -1), ("d_kf_by_order", None), ("d_obs_start", None), ("d_kf_mp", None)):
        v2 = LocalMapView.from_buffer_copy(V)
        setattr(v2, field, v)
        assert call(v=v2) == ORB_E_INVALID, field
    p2 = RefreshParams.from_buffer_copy(nk.params)
    p2.nlevels = 17
    assert call(p=p2) == ORB_E_INVALID
    assert lib.orbm_newkf_workspace_bytes(4, 4, 0) == 0 and lib.orbm_newkf_workspace_bytes(-1, 4, 4) == 0
    # orbm_recent_points_push
    res = ptr(out["result"])
    assert lib.orbm_recent_points_push(ptr(out["sel"]), 4, ptr(rec), ptr(n_rec), 8, res, None) == 0
    assert lib.orbm_recent_points_push(None, 4, ptr(rec), ptr(n_rec), 8, res, None) == ORB_E_INVALID
    assert lib.orbm_recent_points_push(ptr(out["sel"]), -1, ptr(rec), ptr(n_rec), 8, res, None) == ORB_E_INVALID
    assert lib.orbm_recent_points_push(ptr(out["sel"]), 4, ptr(rec), ptr(n_rec), 0, res, None) == ORB_E_INVALID
    # orbm_cull_map_points
    outc = nk.MapPointCulling(dv, dk, 3, rec, n_rec, 64)
    Vc = NewKeyFrame._view(dv, by_order=False)

    def OC(**kw):
        o = MpCullOut(ptr(dv["mp"]).value, ptr(dv["kf_mp"]).value, ptr(outc["code"]).value, ptr(outc["recent"]).value, ptr(outc["n_recent"]).value,
                      ptr(outc["culled"]).value, ptr(outc["n_culled"]).value, ptr(outc["obs_start"]).value, ptr(outc["obs"]).value,
                      ptr(outc["result"]).value, 64, 8)
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    wc = ptr(outc["work"])
    cull = lambda i=I, o=None, fl=0, r=ptr(rec), n=ptr(n_rec): lib.orbm_cull_map_points(ref(Vc), ref(i), None, 3, fl, r, n, ref(o or OC()), wc, None)   # noqa: E731
    assert cull() == 0 and cull(fl=1) == 0
    assert cull(fl=2) == ORB_E_INVALID and cull(r=None) == ORB_E_INVALID and cull(n=None) == ORB_E_INVALID
    for field in ("d_mp", "d_kf_mp", "d_code", "d_recent_out", "d_n_recent_out", "d_culled", "d_n_culled", "d_obs_start_out", "d_obs_out",
                  "d_result"):
        assert cull(o=OC(**{field: None})) == ORB_E_INVALID, field
    for field, v in (("cap_recent", 0), ("cap_obs_out", -1), ("d_recent_out", ptr(rec).value), ("d_obs_start_out", Vc.d_obs_start)):
        assert cull(o=OC(**{field: v})) == ORB_E_INVALID, field
    for field in ("d_ckf", "d_feat", "d_found", "d_visible", "d_first_kf_id"):
        i2 = NewKfIn.from_buffer_copy(I)
        setattr(i2, field, None)
        assert cull(i=i2) == ORB_E_INVALID, field
    # the wrapper's own checks
    with pytest.raises(OrbHipError):
        NewKeyFrame(SF, 0, lib=lib)
    with pytest.raises(OrbHipError):
        nk.ProcessNewKeyFrame(dv, dk, 3, 4, 64, rec[:4], n_rec)
