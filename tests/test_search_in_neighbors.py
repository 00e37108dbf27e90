"""LocalMapping::SearchInNeighbors on the device map (include/orbhip.h "Fusion in the neighbours"): orbm_search_in_neighbors against a literal
Python restatement of LocalMapping.cc:913-1043, ORBmatcher::Fuse (ORBmatcher.cc:1630-1879) with KeyFrame::GetFeaturesInArea, MapPoint::Replace
(MapPoint.cc:286-338), AddObservation (:160-195) and ComputeDistinctiveDescriptors (:372-460), written over dicts and lists as the reference
holds them: mObservations is a dict walked in the rank order of the key frames (std::map<KeyFrame*, .>), Replace recomputes the survivor's
descriptor inside itself, the float steps are numpy float32 / float64 with the rules of DESIGN.md "Map-point projection".

Every output is compared by exact equality.  Where a constructed case names a wrong variant, the case is also run through that deliberately
wrong variant OF THE RESTATEMENT, so that it is known to discriminate."""
import copy
import ctypes
import math

import numpy as np
import pytest

from devarrays import BACKENDS, lib, to_dev, to_dev_plain, to_host  # noqa: F401
from orbhip import KP_DTYPE
from orbhip._abi import (CULL_FEAT_STEREO, CULL_KEYFRAME_DTYPE, FUSENB_BAD_INDEX, FUSENB_CANDIDATE_OVERFLOW, FUSENB_EV_ADD,
                         FUSENB_EV_KF_POINT_REPLACED, FUSENB_EV_LIST_POINT_REPLACED, FUSENB_EV_NOOP_BAD, FUSENB_EV_NOOP_SAME, FUSENB_EVENT_DTYPE,
                         FUSENB_EVENT_OVERFLOW, FUSENB_OBS_OVERFLOW, FUSENB_POSE_DTYPE, FUSENB_R_FLAGS, FUSENB_R_N_CANDIDATES,
                         FUSENB_R_N_CANDIDATES_REQUIRED, FUSENB_R_N_EVENTS, FUSENB_R_N_OBS, FUSENB_R_N_SEL, FUSENB_R_N_TARGETS,
                         FUSENB_R_N_TARGETS_REQUIRED, FUSENB_TARGET_OVERFLOW, FUSENB_UNSORTED, FUSENB_UNSUPPORTED, LM_KF_BAD, LM_KF_PRESENT,
                         LOCALMAP_KEYFRAME_DTYPE, MAP_POINT_DTYPE, MP_BAD, MP_HAS_OBS, MP_VALID, OBS_KF_BAD, OBS_RIGHT, OBSERVATION_DTYPE,
                         ORB_E_CAPACITY, ORB_E_INVALID, REFRESH_MAX_OBS)
from orbhip._lib import OrbHipError
from orbhip.fuse_neighbors import NeighborFusion

f32, f64 = np.float32, np.float64
FX, FY, CX, CY, MBF, TH = f32(200), f32(200), f32(160), f32(120), f32(20), f32(3)
BOUNDS = (f32(0), f32(320), f32(0), f32(240))
GRID = (f32(0), f32(0), f32(64) / f32(320), f32(48) / f32(240))
NLEVELS, SCALE, TH_LOW = 8, f32(1.2), 50
SF = np.ones(NLEVELS, np.float32)
for _i in range(1, NLEVELS):
    SF[_i] = SF[_i - 1] * SCALE
INV_SIGMA2 = (f32(1) / (SF * SF)).astype(np.float32)
LSF = f32(math.log(SCALE))
EV_NAMES = {FUSENB_EV_ADD: "ADD", FUSENB_EV_LIST_POINT_REPLACED: "LIST", FUSENB_EV_KF_POINT_REPLACED: "KF", FUSENB_EV_NOOP_BAD: "BAD",
            FUSENB_EV_NOOP_SAME: "SAME"}
WG = 256   # the lanes of k_fn_apply's workgroup and of the chunks of k_fn_project (csrc/orbm_fuse_neighbors.hip)

_libm = ctypes.CDLL("libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


# ------------------------------------------------------------------------------------------------ a map as the reference holds it
def desc_of(key, flips=()):
    """a 32-byte descriptor: the pattern of `key` with the bits `flips` inverted"""
    d = np.random.default_rng(1000 + key).integers(0, 256, 32, dtype=np.uint8)
    for b in flips:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def KF(feats, Ow=(0.0, 0.0, 0.0), yaw=0.0, **kw):
    """one key frame: feats = [dict(u, v, oct, desc, ur (mvuRight, default -1), mp (point index or None))]"""
    c, s = math.cos(yaw), math.sin(yaw)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], f64)
    Ow = np.asarray(Ow, f64)
    n = len(feats)
    d = dict(id=None, bad=False, prev=None, Rcw=R.astype(f32), tcw=(-R @ Ow).astype(f32), Ow=Ow.astype(f32),
             x=np.array([f["u"] for f in feats], f32), y=np.array([f["v"] for f in feats], f32),
             oct=[int(f.get("oct", 0)) for f in feats], ur=np.array([f.get("ur", -1.0) for f in feats], f32),
             desc=np.array([f["desc"] for f in feats], np.uint8).reshape(n, 32), mp=[f.get("mp") for f in feats], ordered=[], fuse_target=0)
    d["stereo"] = [bool(u >= 0) for u in d["ur"]]   # mvuRight[i] >= 0
    d.update(kw)
    return d


def MP(pos, desc, normal=(0.0, 0.0, 1.0), ratio=1.5, **kw):
    """one map point seen from about the origin: max_distance = ratio * |pos| (PredictScale then gives ceil(log(ratio) / log(1.2)) = 3)"""
    pos = np.asarray(pos, f32)
    dist = f32(np.sqrt(np.sum(pos.astype(f64) ** 2)))
    d = dict(bad=False, valid=True, pos=pos, normal=np.asarray(normal, f32), max_d=f32(ratio) * dist, min_d=f32(0.1), desc=np.array(desc, np.uint8),
             nObs=None, obs={}, found=1, visible=2, replaced=None)
    d.update(kw)
    return d


class World:
    """kfs: KF dicts (None = an empty slot); mps: MP dicts.  obs of a point = {kf: leftIndex}; where not given it is derived from the key
    frames' mp lists (the first feature holding the point), nObs likewise (the weighted count).  order = the key frames by pointer rank."""

    def __init__(self, kfs, mps, order=None, no_obs=()):
        self.kfs, self.mps = kfs, mps
        self.order = list(order) if order is not None else list(range(len(kfs)))
        self.rank = {k: r for r, k in enumerate(self.order)}
        for i, k in enumerate(kfs):
            if k is not None and k["id"] is None:
                k["id"] = 100 + i
        derived = [not m["obs"] for m in mps]
        for k in self.order:
            if kfs[k] is None:
                continue
            for i, p in enumerate(kfs[k]["mp"]):
                if p is not None and 0 <= p < len(mps) and derived[p] and (k, p) not in no_obs and k not in mps[p]["obs"] and not mps[p]["bad"]:
                    mps[p]["obs"][k] = i
        for m in mps:
            if m["nObs"] is None:
                m["nObs"] = sum(2 if kfs[k]["stereo"][i] else 1 for k, i in m["obs"].items())
        self.grids = {}

    def items(self, p, variant=None):
        """mObservations in iteration order"""
        it = list(self.mps[p]["obs"].items())
        return it if variant == "append_order" else sorted(it, key=lambda e: self.rank[e[0]])

    def grid(self, k):
        """KeyFrame::mGrid: AssignFeaturesToGrid with PosInGrid (C round(): half away from zero)"""
        if k not in self.grids:
            K, g = self.kfs[k], {}
            for i in range(len(K["mp"])):
                vx, vy = float((K["x"][i] - GRID[0]) * GRID[2]), float((K["y"][i] - GRID[1]) * GRID[3])
                px = math.floor(vx + 0.5) if vx >= 0 else -math.floor(-vx + 0.5)
                py = math.floor(vy + 0.5) if vy >= 0 else -math.floor(-vy + 0.5)
                if 0 <= px < 64 and 0 <= py < 48:
                    g.setdefault((px, py), []).append(i)
            self.grids[k] = g
        return self.grids[k]


# ------------------------------------------------------------------------------------------------ the restatement
def hamming(a, b):
    return int(np.unpackbits(a ^ b).sum())


def mat_row(R3, X):
    s = f64(0)
    for k in range(3):
        s = s + f64(R3[k]) * f64(X[k])
    return f32(s)


def dot3(a, b):
    s = f64(0)
    for k in range(3):
        s = s + f64(a[k]) * f64(b[k])
    return s


def predict_scale(ratio):
    with np.errstate(all="ignore"):
        c = np.ceil(f32(_libm.logf(float(ratio))) / LSF)
    n = int(c) if np.isfinite(c) else -2 ** 31
    return 0 if n < 0 else min(n, NLEVELS - 1)


def project(K, mp):
    """ORBmatcher.cc:1700-1761 -> (u, v, ur, level, radius), or the name of the gate that rejected"""
    X = mp["pos"]
    xc, yc, zc = [f32(mat_row(K["Rcw"][r], X) + K["tcw"][r]) for r in range(3)]
    if zc < f32(0):
        return "depth"
    with np.errstate(all="ignore"):
        invz = f32(1) / zc
        u, v = f32(f32(FX * xc) / zc + CX), f32(f32(FY * yc) / zc + CY)
    if not (u >= BOUNDS[0] and u < BOUNDS[1] and v >= BOUNDS[2] and v < BOUNDS[3]):
        return "image"
    ur = f32(u - f32(MBF * invz))
    maxD, minD = f32(f32(1.2) * mp["max_d"]), f32(f32(0.8) * mp["min_d"])
    PO = (X - K["Ow"]).astype(f32)
    dist = f32(np.sqrt(dot3(PO, PO)))
    if dist < minD or dist > maxD:
        return "dist"
    if dot3(PO, mp["normal"]) < f64(0.5) * f64(dist):
        return "normal"
    level = predict_scale(f32(mp["max_d"] / dist))
    return u, v, ur, level, f32(TH * SF[level])


def search(W, k, q, d):
    """KeyFrame::GetFeaturesInArea (KeyFrame.cc:810-854) and the candidate loop :1780-1832 -> (bestDist, bestIdx)"""
    K, g = W.kfs[k], W.grid(k)
    u, v, ur, level, r = q
    x0 = max(0, math.floor(f32(f32(u - GRID[0] - r) * GRID[2])))
    x1 = min(63, math.ceil(f32(f32(u - GRID[0] + r) * GRID[2])))
    y0 = max(0, math.floor(f32(f32(v - GRID[1] - r) * GRID[3])))
    y1 = min(47, math.ceil(f32(f32(v - GRID[1] + r) * GRID[3])))
    best, best_idx = 256, -1
    if x0 >= 64 or x1 < 0 or y0 >= 48 or y1 < 0:
        return best, best_idx
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for idx in g.get((ix, iy), ()):
                if not (abs(f32(K["x"][idx] - u)) < r and abs(f32(K["y"][idx] - v)) < r):
                    continue
                lv = K["oct"][idx]
                if lv < level - 1 or lv > level:
                    continue
                ex, ey = f32(u - K["x"][idx]), f32(v - K["y"][idx])
                if K["ur"][idx] >= 0:
                    er = f32(ur - K["ur"][idx])
                    e2 = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er))
                    if f64(f32(e2 * INV_SIGMA2[lv])) > 7.8:
                        continue
                else:
                    e2 = f32(f32(ex * ex) + f32(ey * ey))
                    if f64(f32(e2 * INV_SIGMA2[lv])) > 5.99:
                        continue
                dist = hamming(d, K["desc"][idx])
                if dist < best:
                    best, best_idx = dist, idx
    return best, best_idx


class Restatement:
    def __init__(self, W, cap_targets, cap_candidates, cap_events, cap_obs_out, variant=None):
        self.W, self.variant = W, variant
        self.cap_targets, self.cap_candidates, self.cap_events, self.cap_obs_out = cap_targets, cap_candidates, cap_events, cap_obs_out
        self.events, self.flags, self.stop = [], 0, False
        self.stats = dict(erase=0, changed=set(), cross=0, refresh_overflow=0)

    def compute_distinctive_descriptors(self, p):
        W, mp = self.W, self.W.mps[p]
        if mp["bad"]:
            return
        descs = [W.kfs[k]["desc"][i] for k, i in W.items(p, self.variant) if not W.kfs[k]["bad"]]
        if not descs:
            return
        N = len(descs)
        if N > REFRESH_MAX_OBS:
            self.stats["refresh_overflow"] += 1
            return
        bits = np.unpackbits(np.array(descs), axis=1).astype(np.float32)   # Hamming distances as two products (exact: counts up to 256)
        D = (bits @ (1 - bits).T + (1 - bits) @ bits.T).astype(np.int32)
        med = np.sort(D, axis=1)[:, int(0.5 * (N - 1))]
        best = descs[int(np.argmin(med))].copy()   # (argmin: the first least)
        if not np.array_equal(best, mp["desc"]):
            self.stats["changed"].add(p)
        mp["desc"] = best

    def add_observation(self, p, k, idx):
        mp = self.W.mps[p]
        mp["obs"][k] = idx
        mp["nObs"] += 2 if self.W.kfs[k]["stereo"][idx] else 1

    def replace(self, a, b):
        W = self.W
        if a == b:
            return
        A, B = W.mps[a], W.mps[b]
        obs = W.items(a, self.variant)
        A["obs"], A["bad"], A["replaced"] = {}, True, b
        for k, idx in obs:
            if k not in B["obs"]:
                W.kfs[k]["mp"][idx] = b
                self.add_observation(b, k, idx)
            else:
                W.kfs[k]["mp"][idx] = None
                self.stats["erase"] += 1
        B["found"] += A["found"]
        B["visible"] += A["visible"]
        if self.variant != "no_recompute":
            self.compute_distinctive_descriptors(b)

    def fuse(self, k, lst, call):
        W, K, n_fused = self.W, self.W.kfs[k], 0
        gated = lambda p: p is None or W.mps[p]["bad"] or k in W.mps[p]["obs"]   # noqa: E731
        before = [gated(p) for p in lst]
        for i, p in enumerate(lst):
            if before[i] if self.variant == "gates_before" else gated(p):
                continue
            q = project(K, W.mps[p])
            if isinstance(q, str):
                continue
            if p in self.stats["changed"]:
                self.stats["cross"] += 1
            best, idx = search(W, k, q, W.mps[p]["desc"])
            if best > TH_LOW:
                continue
            if len(self.events) >= self.cap_events:
                self.flags |= FUSENB_EVENT_OVERFLOW
                self.stop = True
                break
            pin = K["mp"][idx]
            if pin is not None:
                if W.mps[pin]["bad"]:
                    kind = FUSENB_EV_NOOP_BAD
                elif pin == p:
                    kind = FUSENB_EV_NOOP_SAME
                elif (W.mps[pin]["nObs"] >= W.mps[p]["nObs"]) if self.variant == "ge" else (W.mps[pin]["nObs"] > W.mps[p]["nObs"]):
                    kind = FUSENB_EV_LIST_POINT_REPLACED
                    self.replace(p, pin)
                else:
                    kind = FUSENB_EV_KF_POINT_REPLACED
                    self.replace(pin, p)
            else:
                kind = FUSENB_EV_ADD
                self.add_observation(p, k, idx)
                K["mp"][idx] = p
            self.events.append((call, k, i, p, idx, -1 if pin is None else pin, kind))
            n_fused += 1
        return n_fused

    def run(self, cur, mono=False, inertial=False, abort=False):
        W, kfs = self.W, self.W.kfs
        cur_id = kfs[cur]["id"]
        targets = []

        def take(k):
            targets.append(k)
            kfs[k]["fuse_target"] = cur_id
        for k in kfs[cur]["ordered"][:20 if mono else 10]:
            if not (kfs[k]["bad"] or kfs[k]["fuse_target"] == cur_id):
                take(k)
        for i in range(len(targets)):
            if self.variant == "break_top" and abort:
                break
            for k in kfs[targets[i]]["ordered"][:20]:
                if not (kfs[k]["bad"] or kfs[k]["fuse_target"] == cur_id or kfs[k]["id"] == cur_id):
                    take(k)
            if abort:
                break
        if inertial:
            k = kfs[cur]["prev"]
            while len(targets) < 20 and k is not None:
                if not (kfs[k]["bad"] or kfs[k]["fuse_target"] == cur_id):
                    take(k)
                k = kfs[k]["prev"]
        self.targets_required, self.candidates, self.candidates_required = len(targets), [], 0
        self.nfused = [0] * (self.cap_targets + 1)
        if len(targets) > self.cap_targets:
            self.flags |= FUSENB_TARGET_OVERFLOW
            self.targets = []
        else:
            self.targets = targets
            lst = list(kfs[cur]["mp"])
            for t, k in enumerate(targets):
                if self.stop:
                    break
                self.nfused[t] = self.fuse(k, lst, t)
            if not abort and not self.stop:
                seen, cands = set(), []
                for k in targets:
                    for p in kfs[k]["mp"]:
                        if p is None or W.mps[p]["bad"] or p in seen:
                            continue
                        seen.add(p)
                        cands.append(p)
                self.candidates_required = len(cands)
                if len(cands) > self.cap_candidates:
                    self.flags |= FUSENB_CANDIDATE_OVERFLOW
                    cands = cands[:self.cap_candidates]
                self.candidates = cands
                self.nfused[len(targets)] = self.fuse(cur, cands, len(targets))
        if self.stats["refresh_overflow"]:
            self.flags |= 64
        self.sel = []
        for p in kfs[cur]["mp"]:
            if p is not None and not W.mps[p]["bad"] and p not in self.sel:
                self.sel.append(p)
        self.n_obs = sum(len(m["obs"]) for m in W.mps)
        if self.n_obs > self.cap_obs_out:
            self.flags |= FUSENB_OBS_OVERFLOW
        return self

    def observable(self):
        """everything a caller can see, as plain Python values (what the wrong variants are compared on)"""
        W = self.W
        return dict(targets=self.targets, marks=[None if k is None else k["fuse_target"] for k in W.kfs], events=self.events, nfused=self.nfused,
                    candidates=self.candidates, kf_mp=[None if k is None else list(k["mp"]) for k in W.kfs],
                    mps=[(m["bad"], m["nObs"], m["found"], m["visible"], m["replaced"], W.items(p), None if m["bad"] else m["desc"].tobytes())
                         for p, m in enumerate(W.mps)], sel=self.sel, flags=self.flags)


def restate(W, cur, caps, variant=None, **mode):
    return Restatement(copy.deepcopy(W), *caps, variant=variant).run(cur, **mode)


# ------------------------------------------------------------------------------------------------ the map on the device
def flatten(W, with_nobs=True, csr=None):
    """-> (view, fuse) numpy dicts for NeighborFusion.SearchInNeighbors; csr: per point an explicit record list [(kf, idx, flags)] replacing the
    rank-ordered one (unsorted rows, rig records, bad indices)"""
    n_kf, n_mp = len(W.kfs), len(W.mps)
    kf = np.zeros(n_kf, LOCALMAP_KEYFRAME_DTYPE)
    kf["parent"], kf["prev"], kf["covis"] = -1, -1, -1
    ckf, pose = np.zeros(n_kf, CULL_KEYFRAME_DTYPE), np.zeros(n_kf, FUSENB_POSE_DTYPE)
    ckf["prev"], ckf["next"] = -1, -1
    rows, feat, kps, ur, descs = [], [], [], [], []
    cap_conn = max([1] + [len(k["ordered"]) for k in W.kfs if k is not None])
    ordered, n_ordered, target = np.full((n_kf, cap_conn), -1, np.int32), np.zeros(n_kf, np.int32), np.zeros(n_kf, np.uint32)
    for i, k in enumerate(W.kfs):
        if k is None:
            continue
        n = len(k["mp"])
        kf[i]["flags"] = LM_KF_PRESENT | (LM_KF_BAD if k["bad"] else 0)
        kf[i]["prev"] = -1 if k["prev"] is None else k["prev"]
        kf[i]["mp_row0"], kf[i]["n_feat"] = len(rows), n
        ckf[i]["id"], ckf[i]["desc_row0"] = k["id"], len(rows)
        pose[i]["Rcw"], pose[i]["tcw"], pose[i]["Ow"] = k["Rcw"].reshape(9), k["tcw"], k["Ow"]
        rows += [-1 if p is None else p for p in k["mp"]]
        feat += [(o & 0x3F) | (CULL_FEAT_STEREO if s else 0) for o, s in zip(k["oct"], k["stereo"])]
        kp = np.zeros(n, KP_DTYPE)
        kp["x"], kp["y"], kp["octave"], kp["size"], kp["class_id"] = k["x"], k["y"], k["oct"], 31.0, -1
        kps.append(kp)
        ur.append(k["ur"])
        descs.append(k["desc"])
        ordered[i, :len(k["ordered"])] = k["ordered"]
        n_ordered[i], target[i] = len(k["ordered"]), k["fuse_target"]
    mp = np.zeros(n_mp, MAP_POINT_DTYPE)
    mp_desc = np.zeros((max(n_mp, 1), 32), np.uint8)
    recs = []
    for p, m in enumerate(W.mps):
        mp[p]["pos"], mp[p]["normal"], mp[p]["min_distance"], mp[p]["max_distance"], mp[p]["desc_row"] = m["pos"], m["normal"], m["min_d"], m["max_d"], p
        mp[p]["flags"] = (MP_VALID if m["valid"] else 0) | (MP_BAD if m["bad"] else 0) | (MP_HAS_OBS if m["nObs"] > 0 else 0)
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
    cat = lambda parts, dt, tail=(): np.concatenate(parts) if parts else np.zeros((0,) + tail, dt)   # noqa: E731
    fuse = dict(ckf=ckf, pose=pose, feat=np.asarray(feat, np.uint8).reshape(-1), kps=cat(kps, KP_DTYPE), u_right=cat(ur, np.float32),
                kf_desc=np.ascontiguousarray(cat(descs, np.uint8, (32,))), ordered_kf=ordered, n_ordered=n_ordered, mp_desc=mp_desc,
                fuse_target=target.view(np.int32), found=np.array([m["found"] for m in W.mps], np.int32),
                visible=np.array([m["visible"] for m in W.mps], np.int32))
    if with_nobs:
        fuse["mp_nobs"] = np.array([m["nObs"] for m in W.mps], np.int32)
    return view, fuse


RECORDS = ("mp", "obs", "kf", "ckf", "pose", "kps")


def upload(view, fuse, backend):
    dev = lambda d: {k: (to_dev(v, backend) if k in RECORDS else to_dev_plain(v, backend)) for k, v in d.items()}   # noqa: E731
    return dev(view), dev(fuse)


def host(a, dtype=None):
    a = to_host(a)
    return a if dtype is None or a.dtype.names else np.ascontiguousarray(a).view(dtype).reshape(-1)


def fusion(L):
    return NeighborFusion((FX, FY, CX, CY), MBF, BOUNDS, GRID, SF, INV_SIGMA2, LSF, th=TH, lib=L)


def caps_of(W, cur, cap_targets=None, cap_candidates=None, cap_events=None, cap_obs_out=None):
    n_feat = max(len(k["mp"]) for k in W.kfs if k is not None)
    total = sum(len(k["mp"]) for k in W.kfs if k is not None)
    n_obs = sum(len(m["obs"]) for m in W.mps)
    return (cap_targets or len(W.kfs), cap_candidates or max(len(W.mps), 1), cap_events or max(2 * total, 1),
            cap_obs_out if cap_obs_out is not None else n_obs + total), n_feat


def compare(R, dv, df, out, cap_feat, caps):
    """every output of the call against the restatement R, by exact equality"""
    W = R.W
    cap_targets, cap_candidates, cap_events, cap_obs_out = caps
    res = host(out["result"])
    nt = len(R.targets)
    assert res[FUSENB_R_FLAGS] == R.flags, (res[FUSENB_R_FLAGS], R.flags)
    assert (res[FUSENB_R_N_TARGETS], res[FUSENB_R_N_TARGETS_REQUIRED]) == (nt, R.targets_required)
    assert (res[FUSENB_R_N_CANDIDATES], res[FUSENB_R_N_CANDIDATES_REQUIRED]) == (len(R.candidates), R.candidates_required)
    assert host(out["targets"])[:nt].tolist() == R.targets
    assert host(out["candidates"])[:len(R.candidates)].tolist() == R.candidates
    assert host(df["fuse_target"]).view(np.uint32).tolist() == [0 if k is None else k["fuse_target"] for k in W.kfs]
    assert res[FUSENB_R_N_EVENTS] == len(R.events)
    ev = host(out["events"], FUSENB_EVENT_DTYPE)[:len(R.events)]
    got = [tuple(int(e[n]) for n in ("call", "kf", "list_index", "point", "feature", "other", "kind")) for e in ev]
    assert got == R.events, [(g, w) for g, w in zip(got, R.events) if g != w][:3]
    assert host(out["nfused"]).tolist() == R.nfused
    want_rows = [-1 if p is None else p for k in W.kfs if k is not None for p in k["mp"]]
    assert host(dv["kf_mp"]).tolist() == want_rows
    mp = host(dv["mp"], MAP_POINT_DTYPE)
    want_flags = [(MP_VALID if m["valid"] else 0) | (MP_BAD if m["bad"] else 0) | (MP_HAS_OBS if m["nObs"] > 0 else 0) for m in W.mps]
    assert mp["flags"].tolist() == want_flags
    if "mp_nobs" in df:
        assert host(df["mp_nobs"]).tolist() == [m["nObs"] for m in W.mps]
    assert host(df["found"]).tolist() == [m["found"] for m in W.mps] and host(df["visible"]).tolist() == [m["visible"] for m in W.mps]
    assert host(out["replaced"])[:len(W.mps)].tolist() == [-1 if m["replaced"] is None else m["replaced"] for m in W.mps]
    assert res[FUSENB_R_N_OBS] == R.n_obs
    if not R.flags & FUSENB_OBS_OVERFLOW:
        row0 = np.concatenate([[0], np.cumsum([0 if k is None else len(k["mp"]) for k in W.kfs])]).tolist()
        want = [[(k, row0[k] + i, OBS_KF_BAD if W.kfs[k]["bad"] else 0) for k, i in W.items(p)] for p in range(len(W.mps))]
        start = host(out["obs_start"])
        assert start.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in want])]).astype(np.int64).tolist()
        obs = host(out["obs"], OBSERVATION_DTYPE)[:R.n_obs]
        assert [(int(o["kf"]), int(o["desc_row"]), int(o["flags"])) for o in obs] == [r for rr in want for r in rr]
    md = host(df["mp_desc"])
    for p, m in enumerate(W.mps):
        if not m["bad"]:
            assert np.array_equal(md[p], m["desc"]), ("descriptor of point", p)
    assert res[FUSENB_R_N_SEL] == len(R.sel)
    assert host(out["sel"]).tolist() == R.sel + [-1] * (cap_feat - len(R.sel))


def run(L, backend, W, cur, with_nobs=True, csr=None, R=None, work=None, **kw):
    mode = {k: kw.pop(k) for k in ("mono", "inertial", "abort") if k in kw}
    caps, cap_feat = caps_of(W, cur, **kw)
    R = R if R is not None else restate(W, cur, caps, **mode)
    view, fuse = flatten(W, with_nobs, csr)
    dv, df = upload(view, fuse, backend)
    nf = fusion(L)
    out = nf.SearchInNeighbors(dv, df, cur, cap_feat, *caps, bMonocular=mode.get("mono", False), bInertial=mode.get("inertial", False),
                               bAbortBA=mode.get("abort", False), work=work)
    compare(R, dv, df, out, cap_feat, caps)
    return R, nf, out


def differs(W, cur, variant, caps=None, **mode):
    """the case discriminates: the wrong variant of the restatement gives another observable result"""
    caps = caps or caps_of(W, cur)[0]
    return restate(W, cur, caps, **mode).observable() != restate(W, cur, caps, variant=variant, **mode).observable()


def kinds(R):
    return [EV_NAMES[e[6]] for e in R.events]


# ------------------------------------------------------------------------------------------------ constructed worlds
# Every key frame stands at the origin looking along z; a point at (x, y, 5) projects to (160 + 40 x, 120 + 40 y), its level is 3 and its
# window +-5.18 pixels; features of octave 3 at the exact pixel pass every gate.
def at(x, y, z=5.0):
    return (x, y, z)


def px(x, y):
    return dict(u=160.0 + 40.0 * x, v=120.0 + 40.0 * y)


def feat(x, y, key, mp=None, flips=(), oct=3, ur=-1.0):
    return dict(px(x, y), oct=oct, desc=desc_of(key, flips), ur=ur, mp=mp)


def chain(W, cur, targets):
    """the current key frame's ordered row = targets; the others have none"""
    W.kfs[cur]["ordered"] = list(targets)
    return W


@pytest.mark.parametrize("backend", BACKENDS)
def test_add_mono_and_stereo(lib, backend):
    """1. the ADD branch on a mono feature (weight 1) and on a stereo feature (weight 2)"""
    ur = float(f32(160.0 + 40.0 * 1.0) - f32(MBF * (f32(1) / f32(5))))   # the point's own ur: er = 0
    W = World([KF([feat(0, 0, 1, mp=0), feat(1, 0, 2, mp=1)]), KF([feat(0, 0, 1), feat(1, 0, 2, ur=ur)])],
              [MP(at(0, 0), desc_of(1)), MP(at(1, 0), desc_of(2))])
    R, _, _ = run(lib, backend, chain(W, 0, [1]), 0)
    assert kinds(R)[:2] == ["ADD", "ADD"] and [W_.get("nObs") for W_ in R.W.mps] == [2, 3]


def tie_world(n_list, n_kf, drift=0, stereo_target=False):
    """point 0 in the current key frame (+ n_list - 1 other observers), point 1 at the same place in the target (+ n_kf - 1 others)"""
    kfs = [KF([feat(0, 0, 1, mp=0)]), KF([feat(0, 0, 1, mp=1, ur=156.0 if stereo_target else -1.0)])]   # (ur of the point: 160 - 20 / 5)
    kfs += [KF([feat(0, 0, 1, mp=0)]) for _ in range(n_list - 1)] + [KF([feat(0, 0, 1, mp=1)]) for _ in range(n_kf - 1)]
    W = World(kfs, [MP(at(0, 0), desc_of(1)), MP(at(0, 0), desc_of(1))])
    W.mps[1]["nObs"] += drift
    return chain(W, 0, [1])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n_list, n_kf, drift, first", [(2, 2, 0, "KF"), (2, 3, 0, "LIST"), (3, 2, 0, "KF"), (2, 2, 1, "LIST"), (2, 3, -1, "KF")])
def test_replace_direction(lib, backend, n_list, n_kf, drift, first):
    """2. the direction of Replace at an nObs tie and with one side greater by one; with d_mp_nobs drifted from the record count the array,
    not the rows, decides.  Wrong variant: >="""
    W = tie_world(n_list, n_kf, drift)
    R, _, _ = run(lib, backend, W, 0)
    assert kinds(R)[0] == first
    if n_list == n_kf + drift:   # the tie
        assert differs(W, 0, "ge")


@pytest.mark.parametrize("backend", BACKENDS)
def test_replace_direction_from_the_record_sum(lib, backend):
    """2b. without d_mp_nobs nObs is the weighted record sum: a stereo record weighs 2"""
    W = tie_world(2, 2, stereo_target=True)
    assert [m["nObs"] for m in W.mps] == [2, 3]
    R, _, _ = run(lib, backend, W, 0, with_nobs=False)
    assert kinds(R)[0] == "LIST"


@pytest.mark.parametrize("backend", BACKENDS)
def test_two_list_points_choose_one_feature(lib, backend):
    """3. the second list point sees the first as pMPinKF"""
    W = World([KF([feat(0, 0, 1, mp=0), feat(0.01, 0, 1, mp=1, flips=(3,))]), KF([feat(0, 0, 1)])],
              [MP(at(0, 0), desc_of(1)), MP(at(0.01, 0), desc_of(1, (3,)))])
    R, _, _ = run(lib, backend, chain(W, 0, [1]), 0)
    assert kinds(R)[:2] == ["ADD", "LIST"] and R.events[1][5] == 0   # (nObs 2 after the ADD against 1)


@pytest.mark.parametrize("backend", BACKENDS)
def test_same_point_twice_in_the_list(lib, backend):
    """4. the second turn of the same point is gated by IsInKeyFrame.  Wrong variant: gates read before the loop"""
    W = World([KF([feat(0, 0, 1, mp=0), feat(2, 0, 5, mp=0)]), KF([feat(0, 0, 1)])], [MP(at(0, 0), desc_of(1))])
    R, _, _ = run(lib, backend, chain(W, 0, [1]), 0)
    assert kinds(R) == ["ADD"] and differs(W, 0, "gates_before")


@pytest.mark.parametrize("backend", BACKENDS)
def test_replace_erase_branch(lib, backend):
    """5. B already observes one of A's key frames: that feature becomes -1 and nObs does not change"""
    W = World([KF([feat(0, 0, 1, mp=0)]), KF([feat(0, 0, 1, mp=1)]), KF([feat(0, 0, 1, mp=0), feat(0.5, 0.5, 1, mp=1)])],
              [MP(at(0, 0), desc_of(1)), MP(at(0, 0), desc_of(1))])
    R, _, _ = run(lib, backend, chain(W, 0, [1]), 0)
    assert kinds(R)[0] == "KF" and R.stats["erase"] == 1 and R.W.kfs[2]["mp"] == [0, None] and R.W.mps[0]["nObs"] == 3


@pytest.mark.parametrize("backend", BACKENDS)
def test_noop_bad_and_same(lib, backend):
    """6. pMPinKF bad, and pMPinKF == pMP without a record: nothing changes, nFused counts both"""
    W = World([KF([feat(0, 0, 1, mp=0), feat(1, 0, 2, mp=1)]), KF([feat(0, 0, 1, mp=2), feat(1, 0, 2, mp=1)])],
              [MP(at(0, 0), desc_of(1)), MP(at(1, 0), desc_of(2)), MP(at(0, 0), desc_of(1), bad=True)], no_obs={(1, 1)})
    before = copy.deepcopy(W)
    R, _, _ = run(lib, backend, chain(W, 0, [1]), 0, abort=True)
    assert kinds(R) == ["BAD", "SAME"] and R.nfused[0] == 2
    assert [k["mp"] for k in R.W.kfs] == [k["mp"] for k in before.kfs]


def cross_world(second):
    """7. target 1 makes list point 0 absorb point 1, whose two other descriptors outvote point 0's own: at target 2 the changed descriptor
    matches feature B (`feature`) or no feature at all (`th_low`)"""
    a, b = desc_of(1), desc_of(1, tuple(range(60)))   # 60 bits apart: medians 20 (a), 20 (the target's, 20 bits from a), 0 (b): b wins
    f2 = [dict(px(0, 0), oct=3, desc=a, mp=None)] + ([dict(px(0.02, 0), oct=3, desc=b, mp=None)] if second == "feature" else [])
    kfs = [KF([feat(0, 0, 1, mp=0)]), KF([dict(px(0, 0), oct=3, desc=desc_of(1, tuple(range(20))), mp=1)]), KF(f2),
           KF([dict(px(0, 0), oct=3, desc=b, mp=1)]), KF([dict(px(0, 0), oct=3, desc=b, mp=1)])]
    W = World(kfs, [MP(at(0, 0), a), MP(at(0, 0), b)])
    W.mps[0]["nObs"] = 5   # the list point survives
    return chain(W, 0, [1, 2])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("second", ["feature", "th_low"])
def test_descriptor_changes_between_targets(lib, backend, second):
    """7. Wrong variant: no recompute between targets"""
    W = cross_world(second)
    R, _, _ = run(lib, backend, W, 0, abort=True)
    assert kinds(R)[0] == "KF" and 0 in R.stats["changed"] and differs(W, 0, "no_recompute", abort=True)
    assert (kinds(R)[1:] == ["ADD"] and R.events[1][4] == 1) if second == "feature" else len(R.events) == 1


@pytest.mark.parametrize("backend", BACKENDS)
def test_replaced_list_point_is_skipped_and_its_replacement_not_searched(lib, backend):
    """8. the list is a copy: point 0 is replaced by point 1 at target 1; at target 2 neither is searched, though point 1 would match there"""
    kfs = [KF([feat(0, 0, 1, mp=0)]), KF([feat(0, 0, 1, mp=1)]), KF([feat(0, 0, 1)]), KF([feat(0, 0, 1, mp=1)])]
    W = chain(World(kfs, [MP(at(0, 0), desc_of(1)), MP(at(0, 0), desc_of(1))]), 0, [1, 2])
    R, _, _ = run(lib, backend, W, 0, abort=True)
    assert kinds(R) == ["LIST"] and R.W.kfs[2]["mp"] == [None] and R.W.kfs[0]["mp"] == [1]


@pytest.mark.parametrize("backend", BACKENDS)
def test_rank_order_decides_the_descriptor_tie(lib, backend):
    """9. merged rows under a d_kf_by_order that is not the identity: three descriptors at equal pairwise medians, the first ROW wins.  Wrong
    variant: append order"""
    d = [desc_of(1), desc_of(1, (0, 1)), desc_of(1, (2, 3))]   # pairwise 2, 2, 4: medians (lower) 2, 2, 2 -> hm: rows [0,2,2] [2,0,4] [2,4,0]
    kfs = [KF([dict(px(0, 0), oct=3, desc=d[0], mp=0)]), KF([dict(px(0, 0), oct=3, desc=d[1], mp=1)]),
           KF([dict(px(0, 0), oct=3, desc=d[2], mp=1)])]
    W = World(kfs, [MP(at(0, 0), d[0]), MP(at(0, 0), d[1])], order=[2, 1, 0])
    W.mps[0]["nObs"] = 9
    R, _, _ = run(lib, backend, chain(W, 0, [1]), 0, abort=True)
    assert kinds(R) == ["KF"] and [k for k, _ in R.W.items(0)] == [2, 1, 0]
    assert differs(W, 0, "append_order", abort=True)


def target_world():
    """10. 26 key frames: 0 current; its ordered row 1..12 with 2 bad and 3 carrying a stale mark; second neighbours with the current id in
    another slot (25), a duplicate across two rows (20), more than 20 entries in a row; a prev chain 24 -> 23 (bad) -> 22 -> ..."""
    kfs = [KF([feat(0, 0, 1, mp=0)]) for _ in range(26)]
    W = World(kfs, [MP(at(0, 0), desc_of(1))])
    kfs[0]["ordered"] = list(range(1, 13))
    kfs[2]["bad"] = True
    kfs[3]["fuse_target"] = kfs[0]["id"]
    kfs[25]["id"] = kfs[0]["id"]
    kfs[1]["ordered"] = [25, 20, 13, 0]
    kfs[4]["ordered"] = [20, 14]
    kfs[5]["ordered"] = [15] * 20 + [16]
    kfs[0]["prev"] = 24
    for k in range(24, 1, -1):
        kfs[k]["prev"] = k - 1
    kfs[23]["bad"] = True
    return W


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mono, inertial", [(False, False), (True, False), (False, True), (True, True)])
def test_targets(lib, backend, mono, inertial):
    W = target_world()
    R, _, _ = run(lib, backend, W, 0, mono=mono, inertial=inertial, cap_targets=26)
    first = [1, 4, 5, 6, 7, 8, 9, 10] + ([11, 12] if mono else [])
    assert R.targets[:len(first)] == first and R.targets[len(first):len(first) + 4] == [20, 13, 14, 15]
    assert 16 not in R.targets[:len(first) + 4]   # the 21st entry of a row is not read
    assert 25 not in R.targets and 2 not in R.targets and 3 not in R.targets
    if inertial:
        assert len(R.targets) == 20 and R.targets[len(first) + 4:len(first) + 6] == [24, 22]
    else:
        assert len(R.targets) == len(first) + 4


@pytest.mark.parametrize("backend", BACKENDS)
def test_abort(lib, backend):
    """11. with the abort flag the first target's second neighbours are added and the later targets' are not; stage 1 runs in full; no stage
    2, no candidates.  Wrong variant: break at the top"""
    kfs = [KF([feat(0, 0, 1, mp=0)])] + [KF([feat(0, 0, 1)]) for _ in range(4)]
    W = World(kfs, [MP(at(0, 0), desc_of(1))])
    kfs[0]["ordered"], kfs[1]["ordered"], kfs[2]["ordered"] = [1, 2], [3], [4]
    R, _, _ = run(lib, backend, W, 0, abort=True)
    assert R.targets == [1, 2, 3] and kinds(R) == ["ADD"] * 3 and R.candidates == [] and R.nfused[:4] == [1, 1, 1, 0]
    assert differs(W, 0, "break_top", abort=True)
    R2, _, _ = run(lib, backend, W, 0)
    assert R2.targets == [1, 2, 3, 4] and R2.candidates == [0]


@pytest.mark.parametrize("backend", BACKENDS)
def test_candidates(lib, backend):
    """12. the first occurrence across targets (point 1), a point that stage 1 moved into a target (point 0: gated in stage 2, it is in the
    current key frame), a candidate that fuses into the current key frame (point 2 -> the free feature)"""
    kfs = [KF([feat(0, 0, 1, mp=0), feat(1, 1, 3)]), KF([feat(0, 0, 1), feat(2, 0, 2, mp=1), feat(1, 1, 3, mp=2)]),
           KF([feat(2, 0, 2, mp=1), feat(-1, 0, 4, mp=3)])]
    W = World(kfs, [MP(at(0, 0), desc_of(1)), MP(at(2, 0), desc_of(2)), MP(at(1, 1), desc_of(3)), MP(at(-1, 0), desc_of(4))])
    R, _, _ = run(lib, backend, chain(W, 0, [1, 2]), 0)
    assert R.candidates == [0, 1, 2, 3] and R.events[-1][:3] == (2, 0, 2) and kinds(R)[-1] == "ADD" and R.nfused[2] == 1


def ulp(x, n):
    return (np.float32(x).view(np.int32) + np.int32(n)).view(np.float32)


@pytest.mark.parametrize("backend", BACKENDS)
def test_gates_at_the_boundaries(lib, backend):
    """13. every gate at its boundary and the ulps either side: u around maxX, dist3D around both distance bounds, PO.Pn around
    0.5 dist3D, max_distance / dist3D around every PredictScale threshold.  Each sweep is shown to hold both outcomes on the restatement
    first; the points then fuse into one target that has a feature of every octave where they land"""
    K = KF([feat(0, 0, 1)])
    mps = []

    def sweep(gate, exact, make):
        got = []
        for n in range(-3, 4):
            mps.append(make(n))
            q = project(K, mps[-1])
            got.append(q if isinstance(q, str) else None)
        assert set(got) == {None, gate}, (gate, got)
        assert got[3] == exact, (gate, got)
    sweep("image", "image", lambda n: MP((float(ulp(4.0, n)), 0.0, 5.0), desc_of(1)))            # u = 200 x / 5 + 160 == maxX at x = 4
    sweep("dist", None, lambda n: MP(at(0, 0), desc_of(1), max_d=ulp(f32(5) / f32(1.2), n)))   # dist3D against 1.2f * max_distance
    sweep("dist", None, lambda n: MP(at(0, 0), desc_of(1), min_d=ulp(f32(5) / f32(0.8), n)))   # dist3D against 0.8f * min_distance
    sweep("normal", None, lambda n: MP(at(0, 0), desc_of(1), normal=(0.0, 0.0, float(ulp(0.5, n)))))   # PO.Pn == 0.5 dist3D passes
    assert any(f32(f32(1.2) * m["max_d"]) == f32(5) for m in mps[7:14]) and any(f32(f32(0.8) * m["min_d"]) == f32(5) for m in mps[14:21])
    th = (ctypes.c_float * 16)()
    assert lib.orbm_predict_scale_thresholds(float(LSF), NLEVELS, th) == 0
    for k in range(NLEVELS - 1):
        trio = [MP(at(0, 0, 4.0), desc_of(1), max_d=f32(ulp(th[k], n) * f32(4))) for n in (-1, 0, 1)]   # dist3D = 4: the ratio is the threshold
        assert [project(K, m)[3] for m in trio] == [k, k + 1, k + 1]
        mps += trio
    cur = KF([dict(px(3, 3), oct=0, desc=desc_of(9), mp=p) for p in range(len(mps))])
    tgt = KF([dict(px(0, 0), oct=o, desc=desc_of(1), mp=None) for o in range(NLEVELS)] + [dict(u=319.0, v=120.0, oct=3, desc=desc_of(1), mp=None)])
    R, _, _ = run(lib, backend, chain(World([cur, tgt], mps), 0, [1]), 0, abort=True)
    assert len(R.events) >= 20


@pytest.mark.parametrize("backend", BACKENDS)
def test_depth_minus_zero(lib, backend):
    """13. z = -0.0f passes the depth test (only z < 0.0f rejects) and leaves the image through x / z = +-inf, as in the reference; the next
    float below is rejected by the depth test.  (R*X sums from +0, so -0 comes from a product that underflows)"""
    tgt = KF([feat(0, 0, 1)])
    tgt["Rcw"][2] = (0, 0, 1e-30)
    tgt["tcw"][2] = f32(-0.0)
    mps = [MP((1.0, 1.0, -1e-30), desc_of(1)), MP((1.0, 1.0, -1.0), desc_of(1)), MP(at(0, 0), desc_of(1))]
    assert [project(tgt, m) for m in mps[:2]] == ["image", "depth"]
    cur = KF([dict(px(3, 3), oct=0, desc=desc_of(9), mp=p) for p in range(3)])
    R, _, _ = run(lib, backend, chain(World([cur, tgt], mps), 0, [1]), 0, abort=True)
    assert [e[3] for e in R.events] == [2]   # (the third point is the control: it lands on the feature)


@pytest.mark.parametrize("backend", BACKENDS)
def test_list_longer_than_a_chunk_and_rows_longer_than_a_wave(lib, backend):
    """14. a list of WG + 1 points: the last (in another chunk) and the first choose one feature, so the serial order crosses the chunk; the
    survivor then has 66 rows, more than one wave"""
    n = WG + 1
    feats = [feat(0, 0, 1, mp=0)] + [dict(px(3, 3), oct=0, desc=desc_of(7), mp=None) for _ in range(n - 2)] + [feat(0.01, 0, 1, mp=1)]
    kfs = [KF(feats), KF([feat(0, 0, 1)])] + [KF([feat(0, 0, 1, mp=1, flips=(k % 32,))]) for k in range(65)]
    W = World(kfs, [MP(at(0, 0), desc_of(1)), MP(at(0.01, 0), desc_of(1))])
    R, _, _ = run(lib, backend, chain(W, 0, [1]), 0, abort=True, cap_targets=2)
    assert kinds(R) == ["ADD", "KF"] and R.events[1][2] == WG and len(R.W.mps[0]["obs"]) == 0 and len(R.W.mps[1]["obs"]) == 67


@pytest.mark.parametrize("backend", BACKENDS)
def test_merged_csr_scans_more_than_256_blocks(lib, backend):
    """14b. 65 536 + 300 point slots, nearly all empty (one dict stands in every empty slot: nothing touches it): 258 blocks of 256 points, so
    the one-workgroup scan of the block totals (csrc/obs_csr.inc) takes a second chunk, whose offsets continue the first's.  The current key
    frame holds six points in blocks on both sides of block 256; the first target holds another point, 65537, where point 3 lands (a
    Replace), the second target nothing: every other turn is an Add.  The slots 10 and 65700 are valid points without records"""
    n_mp = 256 * WG + 300
    pts, xs = [3, 300, 65535, 65536, 65800, n_mp - 1], [-2.5 + j for j in range(6)]
    kfs = [KF([feat(x, 0, 10 + j, mp=p) for j, (x, p) in enumerate(zip(xs, pts))]),
           KF([feat(x, 0, 10 + j, mp=65537 if j == 0 else None) for j, x in enumerate(xs)]), KF([feat(x, 0, 10 + j) for j, x in enumerate(xs)])]
    mps = [MP(at(9, 9), desc_of(0), valid=False)] * n_mp
    for j, (x, p) in enumerate(zip(xs, pts)):
        mps[p] = MP(at(x, 0), desc_of(10 + j))
    mps[65537], mps[10], mps[65700] = MP(at(xs[0], 0), desc_of(10)), MP(at(8, 8), desc_of(98)), MP(at(8, 8), desc_of(99))
    R, _, _ = run(lib, backend, chain(World(kfs, mps), 0, [1, 2]), 0, cap_candidates=16)
    assert kinds(R) == ["KF"] + ["ADD"] * 11 and R.events[0][3] == 3 and R.events[0][5] == 65537
    touched = [e[3] for e in R.events if e[6] == FUSENB_EV_ADD] + [e[5] for e in R.events if e[6] == FUSENB_EV_KF_POINT_REPLACED]
    assert any(p >= 256 * WG for p in touched) and any(p < 256 * WG for p in touched) and R.n_obs == 6 + 1 + 11


def caps_world():
    kfs = [KF([feat(0, 0, 1, mp=0), feat(1, 0, 2, mp=1)])] + [KF([feat(0, 0, 1), feat(1, 0, 2)]) for _ in range(3)]
    W = World(kfs, [MP(at(0, 0), desc_of(1)), MP(at(1, 0), desc_of(2))])
    kfs[0]["ordered"] = [1, 2, 3]
    return W


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("which, full, bit", [("cap_targets", 3, FUSENB_TARGET_OVERFLOW), ("cap_candidates", 2, FUSENB_CANDIDATE_OVERFLOW),
                                              ("cap_events", 6, FUSENB_EVENT_OVERFLOW), ("cap_obs_out", 8, FUSENB_OBS_OVERFLOW)])
def test_capacities_full_and_one_over(lib, backend, which, full, bit):
    """15. every capacity at exactly full and at one over.  Target overflow fuses nothing (the marks are made all the same); candidate
    overflow fuses the first cap_candidates; the turn whose event does not fit is not applied and ends the walk; an observation overflow
    leaves the CSR unwritten.  check_flags() raises ORB_E_CAPACITY"""
    W = caps_world()
    R, nf, out = run(lib, backend, W, 0, **{which: full})
    assert R.flags == 0 and len(R.events) == 6
    nf.check_flags(out)
    R, nf, out = run(lib, backend, W, 0, **{which: full - 1})
    assert R.flags == bit
    if which == "cap_targets":
        assert R.events == [] and [k["fuse_target"] for k in R.W.kfs[1:]] == [100] * 3
    if which == "cap_events":
        assert len(R.events) == 5
    if which == "cap_obs_out":
        sent = host(out["obs_start"]).tolist()
        assert sent == [0] * 3   # never written: as allocated
    with pytest.raises(OrbHipError) as e:
        nf.check_flags(out)
    assert e.value.code == ORB_E_CAPACITY


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("extra", [0, 1])
def test_refresh_max_obs_reached_by_merging(lib, backend, extra):
    """15. a survivor that reaches ORBM_REFRESH_MAX_OBS usable records by merging is recomputed; with one more its descriptor is left
    alone and the call says so.  (Exactly full is a million Hamming distances: the one slow case of the emulated tier, about 12 s)"""
    n = REFRESH_MAX_OBS - 2 + extra   # point 1: the target and n others; the survivor (point 0) adds the current key frame's record
    kfs = [KF([feat(0, 0, 1, mp=0)]), KF([feat(0, 0, 1, mp=1, flips=(1,))])] + [KF([feat(0, 0, 1, mp=1, flips=(2,))]) for _ in range(n)]
    W = World(kfs, [MP(at(0, 0), desc_of(1)), MP(at(0, 0), desc_of(1, (1,)))])
    W.mps[0]["nObs"] = 5000
    R, nf, out = run(lib, backend, chain(W, 0, [1]), 0, abort=True, cap_targets=1)
    assert kinds(R) == ["KF"] and len(R.W.mps[0]["obs"]) == REFRESH_MAX_OBS + extra
    assert R.flags == (64 if extra else 0) and np.array_equal(R.W.mps[0]["desc"], desc_of(1) if extra else desc_of(1, (2,)))
    if extra:
        with pytest.raises(OrbHipError) as e:
            nf.check_flags(out)
        assert e.value.code == ORB_E_CAPACITY


def _far(W, k):
    """key frame k with descriptors nothing matches: what a key frame whose rows cannot be used amounts to in caps_world()"""
    W.kfs[k]["desc"] = np.array([desc_of(900 + i) for i in range(len(W.kfs[k]["mp"]))], np.uint8)


def _no_record(W):
    W.mps[0]["obs"] = {}   # (nObs is the caller's array: it stays)


def _reorder(W):
    W.order = [0, 2, 3, 1]
    W.rank = {k: r for r, k in enumerate(W.order)}


# name -> (corrupt(view, fuse), the same map with the bad entry REMOVED (applied to a copy of the world), flag, inertial)
BAD_INDEX_CASES = {
    "kf_mp": (lambda v, f: v["kf_mp"].__setitem__(3, 77), lambda W: None, FUSENB_BAD_INDEX, False),
    "kf_mp_empty_slot": (lambda v, f: v["kf_mp"].__setitem__(3, 2), lambda W: None, FUSENB_BAD_INDEX, False),
    "ordered_entry": (lambda v, f: f["ordered_kf"].__setitem__((0, 1), 99), lambda W: W.kfs[0].__setitem__("ordered", [1, 3]), FUSENB_BAD_INDEX, False),
    "ordered_count": (lambda v, f: f["n_ordered"].__setitem__(0, 9), lambda W: None, FUSENB_BAD_INDEX, False),
    "record_kf": (lambda v, f: v["obs"]["kf"].__setitem__(0, 50), _no_record, FUSENB_BAD_INDEX, False),
    "record_row": (lambda v, f: v["obs"]["desc_row"].__setitem__(0, 7), _no_record, FUSENB_BAD_INDEX, False),
    "right": (lambda v, f: v["obs"]["flags"].__setitem__(0, OBS_RIGHT), _no_record, FUSENB_UNSUPPORTED, False),
    "csr": (lambda v, f: v["obs_start"].__setitem__(1, 5), lambda W: [m.__setitem__("obs", {}) for m in W.mps], FUSENB_BAD_INDEX, False),
    "by_order": (lambda v, f: v["kf_by_order"].__setitem__(1, 0), _reorder, FUSENB_BAD_INDEX, False),
    "prev_link": (lambda v, f: v["kf"]["prev"].__setitem__(0, 55), lambda W: None, FUSENB_BAD_INDEX, True),
    "n_feat_above_cap_feat": (lambda v, f: v["kf"]["n_feat"].__setitem__(2, 5), lambda W: _far(W, 2), FUSENB_BAD_INDEX, False),
    "desc_row0_outside": (lambda v, f: f["ckf"]["desc_row0"].__setitem__(2, 100), lambda W: _far(W, 2), FUSENB_BAD_INDEX, False),
    "point_desc_row": (lambda v, f: (v["mp"]["desc_row"].__setitem__(1, 99), f["mp_desc"].__setitem__(1, desc_of(99))),
                       lambda W: W.mps[1].__setitem__("desc", desc_of(99)), FUSENB_BAD_INDEX, False),
}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", sorted(BAD_INDEX_CASES))
def test_bad_index_is_flagged_and_absent(lib, backend, name):
    """15. each kind of bad index, and an ORBM_OBS_RIGHT record: flagged, never read through, and treated as absent: every output equals the
    restatement's on the map that has the bad entry REMOVED"""
    corrupt, remove, bit, inertial = BAD_INDEX_CASES[name]
    W = caps_world()
    if name == "kf_mp_empty_slot":
        W.mps.append(MP(at(3, 3), desc_of(5), valid=False, nObs=0))
    caps, cap_feat = caps_of(W, 0)
    view, fuse = flatten(W)
    corrupt(view, fuse)
    W2 = copy.deepcopy(W)
    remove(W2)
    R = restate(W2, 0, caps, inertial=inertial)
    R.flags |= bit
    assert len(R.events) >= 3
    dv, df = upload(view, fuse, backend)
    nf = fusion(lib)
    out = nf.SearchInNeighbors(dv, df, 0, cap_feat, *caps, bInertial=inertial)
    compare(R, dv, df, out, cap_feat, caps)
    with pytest.raises(OrbHipError) as e:
        nf.check_flags(out)
    assert e.value.code == ORB_E_INVALID


@pytest.mark.parametrize("backend", BACKENDS)
def test_bad_current_key_frame_and_overlapping_csr(lib, backend):
    """15. a current key frame that cannot be read: flagged, no target, no event, an empty d_sel.  A d_obs_start that is not monotone, with two
    ranges that are valid each on its own and share a record: flagged, the record is linked once (which point gets it is not specified), and
    the call ends"""
    W = caps_world()
    caps, cap_feat = caps_of(W, 0)
    view, fuse = flatten(W)
    dv, df = upload(view, fuse, backend)
    out = fusion(lib).SearchInNeighbors(dv, df, 9, cap_feat, *caps)
    res = host(out["result"])
    assert res[FUSENB_R_FLAGS] == FUSENB_BAD_INDEX and res[FUSENB_R_N_TARGETS] == 0 and res[FUSENB_R_N_EVENTS] == 0 and (host(out["sel"]) == -1).all()
    W.mps.append(MP(at(3, 3), desc_of(5), nObs=0))
    caps, cap_feat = caps_of(W, 0)
    view, fuse = flatten(W)
    assert view["obs_start"].tolist() == [0, 1, 2, 2]
    view["obs_start"][:] = [0, 2, 1, 2]   # point 0 [0, 2) and point 2 [1, 2) overlap; point 1 [2, 1) is no range
    dv, df = upload(view, fuse, backend)
    out = fusion(lib).SearchInNeighbors(dv, df, 0, cap_feat, *caps)
    res = host(out["result"])
    assert res[FUSENB_R_FLAGS] & FUSENB_BAD_INDEX and res[FUSENB_R_N_TARGETS] == 3
    start = host(out["obs_start"])
    assert start[0] == 0 and (np.diff(start) >= 0).all() and start[-1] == res[FUSENB_R_N_OBS]


@pytest.mark.parametrize("backend", BACKENDS)
def test_unsorted_rows_are_flagged_and_sorted(lib, backend):
    """input rows that are not in rank order: ORBM_FUSENB_UNSORTED, and the outcome of the sorted map"""
    W = tie_world(3, 2)
    caps, cap_feat = caps_of(W, 0)
    R = restate(W, 0, caps)
    R.flags |= FUSENB_UNSORTED
    view, fuse = flatten(W, csr={0: [(k, i, 0) for k, i in reversed(W.items(0))]})
    dv, df = upload(view, fuse, backend)
    out = fusion(lib).SearchInNeighbors(dv, df, 0, cap_feat, *caps)
    compare(R, dv, df, out, cap_feat, caps)


# ------------------------------------------------------------------------------------------------ random worlds
def random_world(seed, pairs=False):
    """<= 12 key frames on a line looking at a cloud of true points, every true point held by one or two map points (so that fusions
    happen), the current key frame last.  -> (world, current, mode).  pairs: a point that only the current key frame holds gets a second
    observer where a free feature of its true point exists, as CreateNewMapPoints leaves it (World.new lists those points)"""
    rng = np.random.default_rng(seed)
    n_kf, n_true = int(rng.integers(4, 13)), int(rng.integers(20, 100))
    true = np.stack([rng.uniform(-3, 4, n_true), rng.uniform(-2, 2, n_true), rng.uniform(4, 8, n_true)], 1)
    tdesc = rng.integers(0, 256, (n_true, 32), dtype=np.uint8)
    toct = rng.integers(1, 5, n_true)
    cams = [(0.25 * i + rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05)) for i in range(n_kf)]
    yaws = [rng.uniform(-0.03, 0.03) for _ in range(n_kf)]
    cur = n_kf - 1
    stereo_kf = [rng.random() < 0.5 for _ in range(n_kf)]
    feats, mps, seen, new = [[] for _ in range(n_kf)], [], [[] for _ in range(n_true)], []
    for k in range(n_kf):
        c, s = math.cos(yaws[k]), math.sin(yaws[k])
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        for j in range(n_true):
            pc = R @ (true[j] - np.array(cams[k]))
            u, v = 200 * pc[0] / pc[2] + 160, 200 * pc[1] / pc[2] + 120
            if not (8 < u < 312 and 8 < v < 232) or rng.random() > 0.75 or len(feats[k]) >= 117:
                continue
            for _ in range(2 if rng.random() < 0.12 else 1):   # (now and then detected twice: two points of one place can share a key frame)
                d = tdesc[j].copy()
                for b in rng.integers(0, 256, int(rng.integers(0, 9))):
                    d[b >> 3] ^= np.uint8(1 << (b & 7))
                ur = u - 20.0 / pc[2] if stereo_kf[k] and rng.random() < 0.8 else -1.0
                seen[j].append((k, len(feats[k])))
                feats[k].append(dict(u=u + rng.uniform(-0.4, 0.4), v=v + rng.uniform(-0.4, 0.4), oct=int(toct[j]), desc=d, ur=ur, mp=None, true=j))
    for j in range(n_true):
        if not seen[j]:
            continue
        inst = {}   # name -> point index
        for k, i in seen[j]:
            r = rng.random()
            if k == cur:
                name = "a" if r < 0.4 else ("c" if r < 0.7 else None)
            else:
                name = None if r < 0.15 else ("a" if r < 0.6 or len(seen[j]) < 3 else "b")
            if name is None:
                continue
            if name not in inst:
                ref = np.array(cams[k])
                dist = np.linalg.norm(true[j] - ref)
                pos = true[j] + rng.uniform(-0.004, 0.004, 3)
                nrm = (true[j] - ref) / dist
                inst[name] = len(mps)
                mps.append(MP(pos, feats[k][i]["desc"], normal=nrm, max_d=f32(dist * float(SF[toct[j]])), min_d=f32(dist * float(SF[toct[j]]) / float(SF[-1])),
                              found=int(rng.integers(1, 9)), visible=int(rng.integers(9, 30)), bad=bool(rng.random() < 0.04)))
            feats[k][i]["mp"] = inst[name]
        free = [(k, i) for k, i in seen[j] if k != cur and feats[k][i]["mp"] is None]
        if pairs and "c" in inst and free:
            feats[free[0][0]][free[0][1]]["mp"] = inst["c"]
            mps[inst["c"]]["bad"] = False
            new.append(inst["c"])
    kfs = [KF(feats[k], Ow=cams[k], yaw=yaws[k], prev=k - 1 if k else None) for k in range(n_kf)]
    no_obs = set()
    for k in range(n_kf):
        for f in feats[k]:
            if f["mp"] is not None and rng.random() < 0.03:
                no_obs.add((k, f["mp"]))
    W = World(kfs, mps, order=list(rng.permutation(n_kf)), no_obs=no_obs)
    W.new = new
    for m in mps:
        if rng.random() < 0.08:
            m["nObs"] += 1   # the drift of MapPoint::nObs
    share = np.zeros((n_kf, n_kf), int)
    for m in mps:
        for a in m["obs"]:
            for b in m["obs"]:
                share[a, b] += a != b
    for k in range(n_kf):
        kfs[k]["ordered"] = [int(o) for o in np.argsort(-share[k], kind="stable") if share[k, o] > 0]
    if rng.random() < 0.2:
        kfs[int(rng.integers(0, n_kf - 1))]["bad"] = True
    return W, cur, dict(mono=bool(rng.random() < 0.5), inertial=bool(rng.random() < 0.3), abort=bool(rng.random() < 0.15))


SEEDS = list(range(24))


@pytest.fixture(scope="module")
def fuzz_worlds():
    """the worlds and their restatements, computed once; non-vacuity is asserted on the restatement alone, before any kernel runs"""
    worlds = []
    for s in SEEDS:
        W, cur, mode = random_world(s)
        caps, cap_feat = caps_of(W, cur)
        worlds.append((W, cur, mode, restate(W, cur, caps, **mode)))
    R = [w[3] for w in worlds]
    seen = {k for r in R for k in kinds(r)}
    assert seen == {"ADD", "LIST", "KF", "BAD", "SAME"}, seen
    assert sum(r.stats["erase"] for r in R) > 0, "the erase branch of Replace"
    assert sum(r.stats["cross"] for r in R) > 0, "a point searched after its descriptor changed"
    assert sum(r.nfused[len(r.targets)] for r in R if r.targets) > 0, "a stage-2 fusion"
    assert sum(1 for r in R if r.events) >= 20
    assert all(len(w[0].kfs) <= 12 and len(w[0].mps) <= 400 and max(len(k["mp"]) for k in w[0].kfs) <= 120 for w in worlds)
    return worlds


def test_fuzz_worlds_are_not_vacuous(fuzz_worlds):
    assert len(fuzz_worlds) == 24


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("i", range(24))
def test_fuzz(lib, backend, fuzz_worlds, i):
    W, cur, mode, R = fuzz_worlds[i]
    run(lib, backend, W, cur, R=R, **mode)


# ------------------------------------------------------------------------------------------------ workspace, refusals, graph
@pytest.mark.parametrize("backend", BACKENDS)
def test_workspace_guard(lib, backend):
    """a workspace of orbm_fusenb_workspace_bytes with canary bytes behind it: the tail is intact after a call that uses every section"""
    from test_workspace_guard import assert_tail_intact, guarded
    W, cur, mode = random_world(3)
    caps, cap_feat = caps_of(W, cur)
    n = lib.orbm_fusenb_workspace_bytes(len(W.kfs), len(W.mps), sum(len(m["obs"]) for m in W.mps), cap_feat, caps[1], caps[2])
    assert n > 0 and n % 16 == 0
    work = guarded(n, backend)
    run(lib, backend, W, cur, work=work, **mode)
    assert_tail_intact(work, n, backend)


def test_workspace_bytes_and_refusals(emu_lib):
    L = emu_lib
    for a in [(-1, 1, 1, 1, 1, 1), (1, -1, 1, 1, 1, 1), (1, 1, -1, 1, 1, 1), (1, 1, 1, 0, 1, 1), (1, 1, 1, 65536, 1, 1), (1, 1, 1, 1, 0, 1),
              (1, 1, 1, 1, 1, 0)]:
        assert L.orbm_fusenb_workspace_bytes(*a) == 0
    assert L.orbm_fusenb_workspace_bytes(0, 0, 0, 1, 1, 1) % 16 == 0 and L.orbm_fusenb_workspace_bytes(5, 7, 9, 3, 4, 2) % 16 == 0
    assert L.orbm_fusenb_workspace_bytes(5, 7, 9, 3, 4, 2) < L.orbm_fusenb_workspace_bytes(5, 7, 9, 3, 4, 20)
    W = caps_world()
    view, fuse = flatten(W)
    nf = fusion(L)
    for bad in (dict(cap_targets=0), dict(cap_events=0), dict(cap_candidates=0), dict(cap_obs_out=-1), dict(cap_feat=0)):
        kw = dict(cap_feat=2, cap_targets=4, cap_candidates=8, cap_events=8, cap_obs_out=16)
        kw.update(bad)
        with pytest.raises(OrbHipError) as e:
            nf.SearchInNeighbors(view, fuse, 0, **kw)
        assert e.value.code == ORB_E_INVALID
    with pytest.raises(OrbHipError):
        nf.SearchInNeighbors(view, fuse, 0, 2, 4, 8, 8, 16, work=np.zeros(16, np.uint8))


@pytest.mark.gpu
def test_graph_capture_replay_hip(hip_lib):
    """the call captured on one stream and replayed twice from restored inputs: the same bytes both times, equal to the eager call"""
    import torch
    W, cur, mode = random_world(5)
    caps, cap_feat = caps_of(W, cur)
    view, fuse = flatten(W)
    dv, df = upload(view, fuse, "hip")
    changed = [(dv, "mp"), (dv, "kf_mp"), (df, "mp_nobs"), (df, "found"), (df, "visible"), (df, "mp_desc"), (df, "fuse_target")]
    keep = [d[k].clone() for d, k in changed]
    nf = fusion(hip_lib)

    def restore():
        for (d, k), v in zip(changed, keep):
            d[k].copy_(v)

    def step(out=None):
        return nf.SearchInNeighbors(dv, df, cur, cap_feat, *caps, bMonocular=mode["mono"], bInertial=mode["inertial"], bAbortBA=mode["abort"], out=out)

    def snapshot(out):
        torch.cuda.synchronize()
        res = out["result"].cpu().numpy()
        cut = dict(targets=res[FUSENB_R_N_TARGETS], candidates=res[FUSENB_R_N_CANDIDATES], events=res[FUSENB_R_N_EVENTS], obs=res[FUSENB_R_N_OBS])
        outs = [out[k].cpu().numpy()[:cut.get(k)].copy() for k in ("targets", "candidates", "nfused", "events", "replaced", "sel", "obs_start", "obs", "result")]
        live = (dv["mp"].cpu().numpy().view(MAP_POINT_DTYPE).reshape(-1)["flags"] & MP_BAD) == 0
        return outs + [d[k].cpu().numpy().copy() for d, k in changed if k != "mp_desc"] + [df["mp_desc"].cpu().numpy()[live].copy()]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = step()   # allocates the outputs and the workspace outside the capture
    torch.cuda.current_stream().wait_stream(s)
    eager = snapshot(out)
    assert eager[8][FUSENB_R_N_EVENTS] >= 1
    restore()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(out)
    for r in range(2):
        restore()
        out["work"].fill_(0x77)
        torch.cuda.synchronize()
        g.replay()
        got = snapshot(out)
        for i, (x, y) in enumerate(zip(got, eager)):
            assert np.array_equal(x, y), (r, i)


# ------------------------------------------------------------------------------------------------ the tail of the reference function
def norm3f(d):
    return f32(np.sqrt(dot3(d, d)))


def normal_and_depth(W, p, ref):
    """MapPoint::UpdateNormalAndDepth (MapPoint.cc:485-558) of point p with mpRefKF / level = ref -> (normal, max_distance, min_distance)"""
    P, rows = W.mps[p], W.items(p)
    normal = np.zeros(3, f32)
    for k, _ in rows:
        d = (P["pos"] - W.kfs[k]["Ow"]).astype(f32)
        normal = (normal + (d / norm3f(d)).astype(f32)).astype(f32)
    dist = norm3f((P["pos"] - W.kfs[int(ref["ref_kf"])]["Ow"]).astype(f32))
    max_d = f32(dist * SF[int(ref["level"])])
    return (normal / f32(len(rows))).astype(f32), max_d, f32(max_d / SF[NLEVELS - 1])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("seed", [0, 9])
def test_fuse_then_refresh_on_one_stream(lib, backend, seed):
    """LocalMapping.cc:1045-1062 right after the fusion, with no host step between: orbm_refresh_map_points(DESCRIPTOR | NORMAL_DEPTH) over
    d_sel, reading the merged CSR and the folded flags where the fusion left them.  The descriptor, the normal and the two distances of
    every point of the current key frame against ComputeDistinctiveDescriptors / UpdateNormalAndDepth (MapPoint.cc:485-558) restated on
    the restatement's final map, bitwise (NaN by class: none arises here)"""
    import orbhip
    from orbhip._abi import KEYFRAME_CENTER_DTYPE, REFRESH_POINT_DTYPE
    W, cur, mode = random_world(seed)
    mode["abort"] = False
    caps, cap_feat = caps_of(W, cur)
    R = restate(W, cur, caps, **mode)
    view, fuse = flatten(W)
    ref = np.zeros(len(W.mps), REFRESH_POINT_DTYPE)
    for p in range(len(W.mps)):   # mpRefKF: the first observer as the map stands (a survivor keeps its own), and that key point's octave
        it = W.items(p)
        ref[p] = (it[0][0], W.kfs[it[0][0]]["oct"][it[0][1]]) if it else (0, 0)
    centers = np.zeros(len(W.kfs), KEYFRAME_CENTER_DTYPE)
    centers["left"] = [k["Ow"] for k in W.kfs]
    dv, df = upload(view, fuse, backend)
    d_ref, d_centers = to_dev(ref, backend), to_dev(centers, backend)
    out = fusion(lib).SearchInNeighbors(dv, df, cur, cap_feat, *caps, bMonocular=mode["mono"], bInertial=mode["inertial"])
    m = orbhip.ORBmatcher(0.8, True, lib=lib)
    m.RefreshMapPoints(dv["mp"], df["mp_desc"], out["obs_start"], out["obs"], d_ref, d_centers, df["kf_desc"], m.RefreshParams(SF), sel=out["sel"])
    assert len(R.sel) >= 5
    mp, md = host(dv["mp"], MAP_POINT_DTYPE), host(df["mp_desc"])
    for p in R.sel:
        R.compute_distinctive_descriptors(p)
        assert np.array_equal(md[p], R.W.mps[p]["desc"]), p
        normal, max_d, min_d = normal_and_depth(R.W, p, ref[p])
        assert mp[p]["normal"].tobytes() == normal.tobytes() and mp[p]["max_distance"] == max_d and mp[p]["min_distance"] == min_d, p


# ------------------------------------------------------------------------------------------------ the whole chain of LocalMapping::Run around it
def renumber(W, keep):
    """the world with its points in the order `keep` (old index per new index)"""
    new_of = {old: new for new, old in enumerate(keep)}
    W.mps = [W.mps[old] for old in keep]
    for k in W.kfs:
        k["mp"] = [None if p is None else new_of[p] for p in k["mp"]]
    for m in W.mps:
        if m["replaced"] is not None:
            m["replaced"] = new_of[m["replaced"]]
    return new_of


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("seed", [4, 17])
def test_chain_append_fuse_refresh_connections_local_map(lib, backend, seed):
    """orbm_append_new_map_points -> orbm_refresh_map_points over the new points (CreateNewMapPoints' ComputeDistinctiveDescriptors /
    UpdateNormalAndDepth, LocalMapping.cc:889-891) -> orbm_search_in_neighbors -> orbm_refresh_map_points over d_sel -> orbm_update_connections
    -> orbm_update_local_map, every call on the slabs the call before left, on one stream, with nothing read or synchronised in between.
    The fusion takes the append's slabs whole (n_mp = cap_mp: the slots behind the cursor hold no point); the graph and the local map take
    the merged CSR and the folded d_mp / d_kf_mp.  Against the restatements: the append and the first refresh are restated into the world
    the fusion's restatement starts from, every output of the fusion as everywhere in this file, the second refresh bitwise, the graph by
    the restatement of tests/test_covisibility.py on the restated final map, the local map against the same entry point on a map built on
    the host from the restatements alone.  (As in the create -> append chain of tests/test_covisibility.py, the key frames' d_kf_mp rows name
    the new points ahead of the append: AddMapPoint's index is cursor + rank, which the caller knows.)"""
    import orbhip
    import test_covisibility as cov
    from orbhip._abi import KEYFRAME_CENTER_DTYPE, NEW_POINT_DTYPE, NEWPT_PAIR_DTYPE, REFRESH_POINT_DTYPE
    from orbhip.covisibility import CovisibilityGraph
    W, cur, mode = random_world(seed, pairs=True)
    mode = dict(mono=mode["mono"], inertial=mode["inertial"], abort=False)
    for k in W.kfs:
        k["bad"] = False
    # the points CreateNewMapPoints made: exactly the current key frame and one neighbour; they go last, in the append's order
    is_new = lambda p: p in W.new and not W.mps[p]["bad"] and len(W.mps[p]["obs"]) == 2 and cur in W.mps[p]["obs"]   # noqa: E731
    kf2_of = lambda p: [k for k in W.mps[p]["obs"] if k != cur][0]   # noqa: E731
    new = sorted([p for p in range(len(W.mps)) if is_new(p)], key=lambda p: (kf2_of(p), W.mps[p]["obs"][cur]))
    new_of = renumber(W, [p for p in range(len(W.mps)) if not is_new(p)] + new)
    new = [new_of[p] for p in new]
    n_old, n_all = len(W.mps) - len(new), len(W.mps)
    assert len(new) >= 5 and new == list(range(n_old, n_all))
    for m in W.mps:
        m["nObs"] = sum(2 if W.kfs[k]["stereo"][i] else 1 for k, i in m["obs"].items())   # no drift: the call sums the records itself
    ref = np.zeros(n_all, REFRESH_POINT_DTYPE)
    for p in range(n_all):
        it = W.items(p)
        ref[p] = (cur, W.kfs[cur]["oct"][W.mps[p]["obs"][cur]]) if p >= n_old else ((it[0][0], W.kfs[it[0][0]]["oct"][it[0][1]]) if it else (0, 0))
    # the restated append + refresh of the new points: what the fusion's restatement starts from
    pre = Restatement(W, 1, 1, 1, 1)
    for p in new:
        W.mps[p]["desc"] = np.full(32, 0xEE, np.uint8)
        pre.compute_distinctive_descriptors(p)
        W.mps[p]["normal"], W.mps[p]["max_d"], W.mps[p]["min_d"] = normal_and_depth(W, p, ref[p])
    caps, cap_feat = caps_of(W, cur)
    R = restate(W, cur, caps, **mode)
    assert any(e[3] >= n_old or e[5] >= n_old for e in R.events), "a new point takes part in a fusion"

    # the device map BEFORE the append: the slabs at their capacity, nothing of the new points but their d_kf_mp entries and found / visible
    view, fuse = flatten(W, with_nobs=False)
    n_obs_old = int(view["obs_start"][n_old])
    ref_dev = ref.copy()
    ref_dev[n_old:] = (-9, -9)
    view["mp"][n_old:] = np.zeros(1, MAP_POINT_DTYPE)[0]
    view["obs"][n_obs_old:] = (-9, -9, 0x5A)
    view["obs_start"][n_old + 1:] = -9
    fuse["mp_desc"][n_old:] = 0x5A
    kf2s = sorted({kf2_of(p) for p in new})
    row0 = np.concatenate([[0], np.cumsum([len(k["mp"]) for k in W.kfs])]).tolist()
    cap_new = max(sum(1 for p in new if kf2_of(p) == k2) for k2 in kf2s)
    created = dict(new=np.zeros((len(kf2s), cap_new), NEW_POINT_DTYPE), nnew=np.zeros(len(kf2s), np.int32))
    pairs = np.zeros(len(kf2s), NEWPT_PAIR_DTYPE)
    for b, k2 in enumerate(kf2s):
        mine = [p for p in new if kf2_of(p) == k2]
        created["nnew"][b] = len(mine)
        for j, p in enumerate(mine):
            created["new"][b, j] = (W.mps[p]["pos"], W.mps[p]["obs"][cur], W.mps[p]["obs"][k2], 1)
        pairs[b]["kf1"], pairs[b]["kf2"], pairs[b]["obs_kf2_first"] = cur, k2, W.rank[k2] < W.rank[cur]
        pairs[b]["desc_row0_1"], pairs[b]["desc_row0_2"] = row0[cur], row0[k2]
    kps1 = np.zeros((len(kf2s), len(W.kfs[cur]["mp"])), KP_DTYPE)
    kps1["octave"] = W.kfs[cur]["oct"]
    centers = np.zeros(len(W.kfs), KEYFRAME_CENTER_DTYPE)
    centers["left"] = [k["Ow"] for k in W.kfs]
    rows = [[p for p in k["mp"]] for k in W.kfs]
    CW = cov.World(rows, n_all, order=W.order, ids=[k["id"] for k in W.kfs])
    _, ckf, st = cov.flatten(CW)

    dv, df = upload(view, fuse, backend)
    d_created = dict(new=to_dev(created["new"], backend), nnew=to_dev_plain(created["nnew"], backend))
    d_pairs, d_kps1, d_ref, d_centers = to_dev(pairs, backend), to_dev(kps1, backend), to_dev(ref_dev, backend), to_dev(centers, backend)
    d_nmp, d_list = to_dev_plain(np.asarray([n_old], np.int32), backend), to_dev_plain(np.asarray([cur], np.int32), backend)
    d_ckf = cov.rec_dev(ckf, backend)
    d_st = {k: (cov.rec_dev(v, backend) if v.dtype.names else to_dev_plain(v.copy(), backend)) for k, v in st.items()}
    votes = [p for p in R.sel][:30]
    lm_view = cov.with_local_map_arrays(dv, backend)
    d_vote = None
    m, nf, G = orbhip.ORBmatcher(0.8, True, lib=lib), fusion(lib), CovisibilityGraph(d_st, d_ckf, lib=lib)
    prm = m.RefreshParams(SF)
    a = np.full((1, len(votes) + 3), -1, np.int32)
    a[0, :len(votes)] = votes
    fr = np.zeros(1, cov.LOCALMAP_FRAME_DTYPE)
    fr["last_kf"] = -1
    d_vote = (to_dev_plain(a, backend), to_dev_plain(np.asarray([len(votes)], np.int32), backend), to_dev(fr, backend))

    # ---- the chain: nothing is read back or synchronised until it ends
    app = m.AppendNewMapPoints(d_created, d_pairs, d_kps1, d_nmp, dv["mp"], n_all, dv["obs_start"], dv["obs"], d_ref, len(new) + 3)
    m.RefreshMapPoints(dv["mp"], df["mp_desc"], dv["obs_start"], dv["obs"], d_ref, d_centers, df["kf_desc"], prm, sel=app["sel"])
    out = nf.SearchInNeighbors(dv, df, cur, cap_feat, *caps, bMonocular=mode["mono"], bInertial=mode["inertial"])
    m.RefreshMapPoints(dv["mp"], df["mp_desc"], out["obs_start"], out["obs"], d_ref, d_centers, df["kf_desc"], prm, sel=out["sel"])
    merged = dict(lm_view, obs_start=out["obs_start"], obs=out["obs"])
    cv = G.UpdateConnections(merged, d_list, cov.INIT_NONE)
    local, _ = cov.local_map(m, backend, merged, None, d_vote=d_vote)
    cov.sync(backend)

    # ---- the append, as the fusion found it
    assert host(app["appended"]).tolist() == [len(new), 0] and host(d_nmp).tolist() == [n_all]
    assert host(app["sel"]).tolist() == new + [-1] * 3
    assert np.array_equal(cov.u8(host(d_ref)), cov.u8(ref))
    # ---- the fusion and the refresh after it
    for p in R.sel:
        R.compute_distinctive_descriptors(p)
    compare(R, dv, df, out, cap_feat, caps)
    mp, FW = host(dv["mp"], MAP_POINT_DTYPE), R.W
    for p in R.sel:
        normal, max_d, min_d = normal_and_depth(FW, p, ref[p])
        assert mp[p]["normal"].tobytes() == normal.tobytes() and mp[p]["max_distance"] == max_d and mp[p]["min_distance"] == min_d, p
    for p in new:   # a new point that no refresh touched again keeps what the first refresh gave it
        if p not in R.sel and not FW.mps[p]["bad"]:
            assert mp[p]["normal"].tobytes() == W.mps[p]["normal"].tobytes() and mp[p]["max_distance"] == W.mps[p]["max_d"], p
    # ---- the graph: KeyFrame::UpdateConnections restated on the restated final map
    CF = cov.World([list(k["mp"]) for k in FW.kfs], n_all, order=W.order, ids=[k["id"] for k in FW.kfs], bad_mp=[p for p in range(n_all) if FW.mps[p]["bad"]])
    for p in range(n_all):
        CF.mps[p]["obs"] = [k for k, _ in FW.items(p)]
    view_cf, _, _ = cov.flatten(CF)
    res = cov.update_connections(CF, cur, cov.INIT_NONE)
    assert res["n_counter"] >= 3
    assert [int(host(cv[k])[0]) for k in ("nmax", "kfmax", "n_counter", "flags", "n_child_events")] == [res["nmax"], res["kfmax"], res["n_counter"], 0, 1]
    view0 = dict(mp=cov.as_rec(dv["mp"], MAP_POINT_DTYPE), obs_start=host(out["obs_start"]).copy(), obs=cov.as_rec(out["obs"], OBSERVATION_DTYPE),
                 kf=view["kf"], kf_mp=host(dv["kf_mp"]).copy(), kf_by_order=view["kf_by_order"])
    cov.check_store(CF, view0, ckf, st, merged, d_ckf, d_st)
    # ---- the local map: the same entry point on a map built on the host from the restatements alone
    got = cov.local_map_result(m, local)
    kf_want = view["kf"].copy()
    for k, K in enumerate(CF.kfs):
        kf_want[k]["covis"] = (K["okf"][:10] + [-1] * 10)[:10]
        kf_want[k]["parent"] = -1 if K["parent"] is None else K["parent"]
    start_want = np.concatenate([[0], np.cumsum([len(FW.mps[p]["obs"]) for p in range(n_all)])]).astype(np.int32)
    obs_want = np.zeros(int(start_want[-1]), OBSERVATION_DTYPE)
    for j, r in enumerate([(k, row0[k] + i, 0) for p in range(n_all) for k, i in FW.items(p)]):
        obs_want[j] = r
    mp_want = mp.copy()
    mp_want["flags"] = [MP_VALID | (MP_BAD if q["bad"] else 0) | (MP_HAS_OBS if q["nObs"] > 0 else 0) for q in FW.mps]
    host_view = dict(mp=to_dev(mp_want, backend), obs_start=to_dev_plain(start_want, backend), obs=cov.rec_dev(obs_want, backend),
                     kf=cov.rec_dev(kf_want, backend), kf_mp=to_dev_plain(np.asarray([-1 if p is None else p for k in FW.kfs for p in k["mp"]], np.int32), backend),
                     kf_by_order=to_dev_plain(view["kf_by_order"].copy(), backend))
    want, _ = cov.local_map(m, backend, cov.with_local_map_arrays(host_view, backend), votes)
    cov.sync(backend)
    want = cov.local_map_result(m, want)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and got[2][1] >= 3 and got[2][2] > 20
