"""Optimizer::LocalBundleAdjustment on the device map (include/orbhip.h "Local bundle adjustment on the device map"): orbm_lba_window_build and
orbm_lba_window_apply against a serial Python restatement of Optimizer.cc:1816-1945, :1978-2190 and :2293-2510 (with the two guards of
integration/Optimizer_hip.cc) over dicts and lists as the reference holds them: mObservations is a dict walked in the rank order of the key
frames (std::map<KeyFrame*, .>), the loops are serial, UpdateNormalAndDepth is the numpy restatement of tests/test_map_refresh.py, and the
solver's CSRs come from orbhip.lba.build_structure.

Every output is compared by exact equality: every slab as bytes, every index, flag and result word.  chi2 and depth of the apply cases are
given by the test, so no solver is involved there; the chain case runs the solver between the two halves and holds it against the oracle."""
import copy

import numpy as np
import pytest

from devarrays import BACKENDS, lib, to_dev, to_dev_plain, to_host  # noqa: F401
from orbhip import KP_DTYPE
from orbhip._abi import (CAM_DTYPE, CAM_PINHOLE, COVIS_KEYFRAME_DTYPE, CULL_FEAT_STEREO, CULL_KEYFRAME_DTYPE, CULL_PROBLEM_DTYPE, EDGE_DTYPE,
                         EDGE_MONO, EDGE_STEREO, FUSENB_POSE_DTYPE, KEYFRAME_CENTER_DTYPE, LBA_A_FLAGS, LBA_A_N_ERASED, LBA_A_N_MONO,
                         LBA_A_N_OBS, LBA_A_N_STEREO, LBA_A_N_WENT_BAD, LBA_A_WORDS, LBA_BAD_INDEX, LBA_EARLY_RETURN, LBA_OVERFLOW,
                         LBA_R_FLAGS, LBA_R_N_EDGES, LBA_R_N_EDGES_REQUIRED, LBA_R_N_FIXED, LBA_R_N_LOCAL, LBA_R_N_MONO, LBA_R_N_POINTS,
                         LBA_R_N_POINTS_REQUIRED, LBA_R_N_POSES_REQUIRED, LBA_R_N_STEREO, LBA_R_NUM_FIXED_KF, LBA_R_WORDS,
                         LBA_UNSUPPORTED, LM_KF_BAD, LM_KF_PRESENT, LOCALMAP_KEYFRAME_DTYPE, MAP_POINT_DTYPE, MP_BAD, MP_HAS_OBS, MP_VALID,
                         OBS_KF_BAD, OBS_RIGHT, OBSERVATION_DTYPE, ORB_E_CAPACITY, ORB_E_INVALID, REFRESH_POINT_DTYPE)
from orbhip._lib import OrbHipError
from orbhip.lba import HUBER_MONO, HUBER_STEREO, build_structure
from orbhip.local_ba import LocalBA
from test_map_refresh import normal_and_depth

f32, f64 = np.float32, np.float64
NLEVELS = 8
SF = np.ones(NLEVELS, f32)
for _i in range(1, NLEVELS):
    SF[_i] = SF[_i - 1] * f32(1.2)
INV_SIGMA2 = (f32(1.0) / (SF * SF)).astype(f32)
FX, FY, CX, CY, BF = 458.654, 457.296, 367.215, 248.375, 47.906
CAM = np.zeros(1, CAM_DTYPE)
CAM[0]["model"] = CAM_PINHOLE
CAM[0]["p"][:4] = f32([FX, FY, CX, CY])
CAM[0]["bf"] = f32(BF)
CAM[0]["trl_q"] = [0, 0, 0, 1]
FILL = 0x5A   # what the window slabs hold before a call: an overflow must leave it


# ------------------------------------------------------------------------------------------------ a map as the reference holds it
def KF(mp, u_right=None, oct=None, xy=None, R=None, t=(0.0, 0.0, 0.0), **kw):
    """one key frame: mp = GetMapPointMatches() as point indices (None = null)"""
    n = len(mp)
    d = dict(id=None, bad=False, map=0, mp=list(mp), u_right=[f32(-1)] * n if u_right is None else [f32(u) for u in u_right],
             oct=[0] * n if oct is None else list(oct), xy=[(f32(10 * j), f32(5 * j + 1)) for j in range(n)] if xy is None else list(xy),
             R=np.eye(3, dtype=f32) if R is None else np.asarray(R, f32), t=np.asarray(t, f32), covis=[])
    d.update(kw)
    d["center"] = d.get("center", ow_gemm(d["R"], d["t"]))
    return d


def MP(pos=(0.0, 0.0, 5.0), **kw):
    d = dict(valid=True, bad=False, pos=np.asarray(pos, f32), normal=np.array([0, 0, 1], f32), min_d=f32(1), max_d=f32(9), nObs=None, obs={},
             ref_kf=None, level=0)
    d.update(kw)
    d["obs"] = dict(d["obs"])
    return d


class World:
    """kfs: KF dicts (None = an empty slot); mps: MP dicts; obs of a point = {kf: leftIndex}; order = the key frames by pointer rank;
    kf["covis"] = GetVectorCovisibleKeyFrames()."""

    def __init__(self, kfs, mps, order=None):
        self.kfs, self.mps = kfs, mps
        self.order = list(order) if order is not None else list(range(len(kfs)))
        self.rank = {k: r for r, k in enumerate(self.order)}
        for i, k in enumerate(kfs):
            if k is not None and k["id"] is None:
                k["id"] = 100 + i
        for m in mps:
            if m["nObs"] is None:
                m["nObs"] = self.weight_sum(m)
            if m["ref_kf"] is None:
                m["ref_kf"] = self.items_of(m)[0][0] if m["obs"] else 0

    def weight_sum(self, m):
        return sum(2 if self.kfs[k]["u_right"][i] >= 0 else 1 for k, i in m["obs"].items())

    def items_of(self, m):
        return sorted(m["obs"].items(), key=lambda e: self.rank[e[0]])

    def items(self, p):
        """mObservations in iteration order"""
        return self.items_of(self.mps[p])


def link(W):
    """the obs dicts from the key frames' rows: the first feature of a key frame that holds a point is its record"""
    for m in W.mps:
        m["obs"] = {}
    for k, kf in enumerate(W.kfs):
        if kf is None:
            continue
        for i, p in enumerate(kf["mp"]):
            if p is not None and k not in W.mps[p]["obs"]:
                W.mps[p]["obs"][k] = i
    for m in W.mps:
        m["nObs"] = W.weight_sum(m)
        m["ref_kf"] = W.items_of(m)[0][0] if m["obs"] else 0
    return W


# ------------------------------------------------------------------------------------------------ the float rules
def pose_from_tcw(R, t):
    """LbaLinearizer::poseFromTcw: Eigen Quaterniond(Matrix3d) + SE3Quat::normalizeRotation, in double from the float matrix"""
    m = [f64(v) for v in np.asarray(R, f32).reshape(9)]
    q = [f64(0)] * 4
    tr = m[0] + m[4] + m[8]
    if tr > 0:
        tr = np.sqrt(tr + f64(1.0)); q[3] = f64(0.5) * tr; tr = f64(0.5) / tr
        q[0] = (m[7] - m[5]) * tr; q[1] = (m[2] - m[6]) * tr; q[2] = (m[3] - m[1]) * tr
    else:
        i = 0
        if m[4] > m[0]:
            i = 1
        if m[8] > m[i * 3 + i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        tr = np.sqrt(m[i * 3 + i] - m[j * 3 + j] - m[k * 3 + k] + f64(1.0))
        q[i] = f64(0.5) * tr
        tr = f64(0.5) / tr
        q[3] = (m[k * 3 + j] - m[j * 3 + k]) * tr; q[j] = (m[j * 3 + i] + m[i * 3 + j]) * tr; q[k] = (m[k * 3 + i] + m[i * 3 + k]) * tr
    if q[3] < 0:
        q = [-v for v in q]
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return np.array([f64(v) for v in np.asarray(t, f32)] + [v / n for v in q], f64)


def ow_gemm(R, t, variant=None):
    """Ow = -Rwc * tcw as one cv::gemm with alpha = -1: a double sum of double products in k order, times alpha, rounded once"""
    R, t = np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32)
    ow = np.zeros(3, f32)
    for r in range(3):
        if variant == "float_sum":   # the wrong variant: float accumulation
            s = f32(R[0, r] * t[0])
            s = f32(s + f32(R[1, r] * t[1]))
            s = f32(s + f32(R[2, r] * t[2]))
            ow[r] = -s
        else:
            s = f64(R[0, r]) * f64(t[0])
            s = s + f64(R[1, r]) * f64(t[1])
            s = s + f64(R[2, r]) * f64(t[2])
            ow[r] = f32(s * f64(-1.0))
    return ow


def pose_to_float(p7):
    """Converter::toCvMat(SE3Quat): Rcw | tcw as floats of to_homogeneous_matrix in double"""
    x, y, z, w = [f64(v) for v in p7[3:]]
    one, two = f64(1), f64(2)
    R = [one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w), two * (x * y + z * w), one - two * (x * x + z * z),
         two * (y * z - x * w), two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]
    return np.array(R, f64).astype(f32).reshape(3, 3), np.asarray(p7[:3], f64).astype(f32)


def int32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


# ------------------------------------------------------------------------------------------------ the map on the device
def flatten(W, csr=None, kf_mp_raw=None, covis_raw=None, cap_conn=None, use_map=True, kf_rows=None, obs_start_raw=None, n_ordered_raw=None):
    """-> (view, kfs, records) numpy dicts for LocalBA; records[p] = [(kf, idx, flags)] as the CSR holds them.  csr: per point an explicit
    record list replacing the rank-ordered one; kf_mp_raw: {(kf, i): raw entry}; covis_raw: {kf: raw row}"""
    n_kf, n_mp = len(W.kfs), len(W.mps)
    kf = np.zeros(n_kf, LOCALMAP_KEYFRAME_DTYPE)
    kf["parent"], kf["prev"], kf["covis"] = -1, -1, -1
    ckf, center, pose = np.zeros(n_kf, CULL_KEYFRAME_DTYPE), np.zeros(n_kf, KEYFRAME_CENTER_DTYPE), np.zeros(n_kf, FUSENB_POSE_DTYPE)
    cmap = np.zeros(n_kf, COVIS_KEYFRAME_DTYPE)
    rows, kps_l, ur = [], [], []
    rowsets = [(covis_raw or {}).get(i, k["covis"] if k is not None else []) for i, k in enumerate(W.kfs)]
    cap_conn = cap_conn or max([len(r) for r in rowsets] + [1])
    ordered, n_ordered = np.full((n_kf, cap_conn), -9, np.int32), np.zeros(n_kf, np.int32)
    for i, k in enumerate(W.kfs):
        if k is None:
            continue
        kf[i]["flags"] = LM_KF_PRESENT | (LM_KF_BAD if k["bad"] else 0)
        kf[i]["mp_row0"], kf[i]["n_feat"] = len(rows), len(k["mp"])
        ckf[i]["id"], ckf[i]["desc_row0"] = k["id"] & 0xFFFFFFFF, len(rows) + 7   # (descriptor rows need not start where the features do)
        cmap[i]["id"], cmap[i]["map_id"] = ckf[i]["id"], k["map"]
        center[i]["left"], center[i]["right"] = k["center"], [7, 7, 7]
        pose[i]["Rcw"], pose[i]["tcw"], pose[i]["Ow"] = k["R"].reshape(9), k["t"], k["center"]
        rows += [(kf_mp_raw or {}).get((i, j), -1 if p is None else p) for j, p in enumerate(k["mp"])]
        for j in range(len(k["mp"])):
            kp = np.zeros(1, KP_DTYPE)
            kp["x"], kp["y"], kp["octave"], kp["size"] = k["xy"][j][0], k["xy"][j][1], k["oct"][j], 31
            kps_l.append(kp)
        ur += k["u_right"]
        ordered[i, :len(rowsets[i])], n_ordered[i] = rowsets[i], len(rowsets[i])
    mp, ref = np.zeros(n_mp, MAP_POINT_DTYPE), np.zeros(n_mp, REFRESH_POINT_DTYPE)
    recs = []
    for p, m in enumerate(W.mps):
        mp[p]["pos"], mp[p]["normal"], mp[p]["min_distance"], mp[p]["max_distance"], mp[p]["desc_row"] = m["pos"], m["normal"], m["min_d"], m["max_d"], p
        mp[p]["flags"] = (MP_VALID if m["valid"] else 0) | (MP_BAD if m["bad"] else 0) | (MP_HAS_OBS if m["nObs"] > 0 else 0)
        ref[p]["ref_kf"], ref[p]["level"] = m["ref_kf"], m["level"]
        recs.append(list(csr[p]) if csr is not None and p in csr else [(k, i, OBS_KF_BAD if W.kfs[k]["bad"] else 0) for k, i in W.items(p)])
    start = np.zeros(n_mp + 1, np.int32)
    start[1:] = np.cumsum([len(r) for r in recs])
    obs = np.zeros(int(start[-1]), OBSERVATION_DTYPE)
    for j, (k, i, fl) in enumerate([r for rr in recs for r in rr]):
        obs[j] = (k, (int(ckf[k]["desc_row0"]) if 0 <= k < n_kf else 0) + i, fl)
    for k, (r0, nf) in (kf_rows or {}).items():                # a key frame's rows as the map names them (they may leave the table)
        kf[k]["mp_row0"], kf[k]["n_feat"] = r0, nf
    for i, v in (obs_start_raw or {}).items():
        start[i] = v
    for k, n in (n_ordered_raw or {}).items():
        n_ordered[k] = n
    view = dict(mp=mp, obs_start=start, obs=obs, kf=kf, kf_mp=np.asarray(rows, np.int32).reshape(-1))
    kfs = dict(ckf=ckf, pose=pose, center=center, ref=ref, kps=np.concatenate(kps_l) if kps_l else np.zeros(0, KP_DTYPE),
               u_right=np.asarray(ur, f32).reshape(-1), ordered_kf=ordered, n_ordered=n_ordered,
               mp_nobs=np.array([m["nObs"] for m in W.mps], np.int32))
    if use_map:
        kfs["map"] = cmap
    return view, kfs, recs


RECORDS = ("mp", "obs", "kf", "ckf", "ref", "center", "pose", "kps", "map")


def rec_dev(a, backend):
    return to_dev(a, backend) if a.size or backend == "emu" else to_dev_plain(np.zeros((0, a.dtype.itemsize), np.uint8), backend)


def upload(view, kfs, backend):
    dev = lambda d: {k: (rec_dev(v, backend) if k in RECORDS else to_dev_plain(v, backend)) for k, v in d.items()}   # noqa: E731
    return dev(copy.deepcopy(view)), dev(copy.deepcopy(kfs))


def host(a, dtype=None):
    a = to_host(a)
    return a if dtype is None or a.dtype.names else np.ascontiguousarray(a).view(dtype).reshape(-1)


def fill(win):
    """every slab of a window set to FILL bytes"""
    for k, a in win.items():
        if k == "work":
            continue
        if isinstance(a, np.ndarray):
            a.view(np.uint8)[...] = FILL
        else:
            import torch
            a.view(torch.uint8).fill_(FILL)


# ------------------------------------------------------------------------------------------------ the restatement: the build
class Result:
    pass


def usable(W, rec, R):
    """the record check of every map-side call -> (kf, idx) or None; what cannot be read is flagged"""
    k, i, fl = rec
    if fl & OBS_RIGHT:
        R.flags |= LBA_UNSUPPORTED
        return None
    rows_of = getattr(R, "rows_of", None)
    if not 0 <= k < len(W.kfs) or W.kfs[k] is None or (rows_of is not None and rows_of(k) is None) or \
            not 0 <= i < (rows_of(k)[1] if rows_of is not None else len(W.kfs[k]["mp"])) or not 0 <= i < len(W.kfs[k]["mp"]):
        R.flags |= LBA_BAD_INDEX
        return None
    return k, i


def restate_build(W, recs, cur, init_id, caps, kf_mp_raw=None, covis_raw=None, variant=None, view=None):
    """Optimizer.cc:1816-1945 and :1978-2190 as integration/Optimizer_hip.cc:58-177 states them, serially"""
    R = Result()
    R.flags, R.overflow = 0, False
    R.llist, R.points, R.fixed, R.edges, R.edge_rec, R.vertices = [], [], [], [], [], []
    R.num_fixed = 0
    n_kf, n_mp = len(W.kfs), len(W.mps)
    present = lambda k: 0 <= k < n_kf and W.kfs[k] is not None   # noqa: E731
    # the tables as the map gives them, where the case damaged them: a key frame's rows, a point's CSR range, the row count
    n_rows = len(view["kf_mp"]) if view is not None else None

    def rows_of(k):
        """(mp_row0, n_feat) of a present key frame, or None where the rows leave the table"""
        if view is None:
            return 0, len(W.kfs[k]["mp"])
        r0, nf = int(view["kf"][k]["mp_row0"]), int(view["kf"][k]["n_feat"])
        return (r0, nf) if r0 >= 0 and nf >= 0 and nf <= n_rows - r0 else None

    def range_ok(p):
        if view is None:
            return True
        s_, e_ = int(view["obs_start"][p]), int(view["obs_start"][p + 1])
        return s_ >= 0 and e_ >= s_ and e_ <= len(view["obs"])
    R.rows_of = rows_of
    if not present(cur) or rows_of(cur) is None:
        R.flags |= LBA_BAD_INDEX
        return finish_build(W, R, init_id, caps)
    pKF = W.kfs[cur]
    in_graph = lambda k: not W.kfs[k]["bad"] and W.kfs[k]["map"] == pKF["map"]   # noqa: E731
    # ---- Local KeyFrames (:1813-1829)
    R.llist.append(cur)
    marked = {cur}
    row = list((covis_raw or {}).get(cur, pKF["covis"]))
    if view is not None:                                        # the count as the map gives it, clamped to the row and flagged
        n_raw = int(view_n_ordered(view, cur))
        cap = view["_cap_conn"]
        if not 0 <= n_raw <= cap:
            R.flags |= LBA_BAD_INDEX
        row = (row + [-9] * cap)[:min(max(n_raw, 0), cap)]
    for k in row:
        if not present(k):
            R.flags |= LBA_BAD_INDEX
            continue
        if k in marked:
            continue
        marked.add(k)
        if in_graph(k):
            R.llist.append(k)
    # ---- Local MapPoints (:1831-1862)
    seen, n_pos = set(), 0
    for k in R.llist:
        if rows_of(k) is None:
            R.flags |= LBA_BAD_INDEX
            continue
        if view is not None:
            r0, nf = rows_of(k)
            feats = [int(v) for v in view["kf_mp"][r0:r0 + nf]]
        else:
            feats = [(kf_mp_raw or {}).get((k, i), -1 if p is None else p) for i, p in enumerate(W.kfs[k]["mp"])]
        for i, p in enumerate(feats):
            n_pos += 1
            if n_rows is not None and n_pos > n_rows:           # more feature positions than the table has rows: the rest is dropped
                R.flags |= LBA_BAD_INDEX
                break
            if p == -1:
                continue
            if not 0 <= p < n_mp or not W.mps[p]["valid"]:
                R.flags |= LBA_BAD_INDEX
                continue
            if W.mps[p]["bad"] or p in seen:
                continue
            seen.add(p)
            R.points.append(p)
    # ---- Fixed Keyframes (:1864-1882) and, in the same walk, the records that become edges
    fixed, per_point = set(), []
    starts = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    for p in R.points:
        mine = []
        if not range_ok(p):
            R.flags |= LBA_BAD_INDEX
        for j, rec in enumerate(recs[p] if range_ok(p) else []):
            u = usable(W, rec, R)
            if u is None or not in_graph(u[0]):
                continue
            k, i = u
            if k not in marked and k not in fixed:
                fixed.add(k)
                R.fixed.append(k)
            if not 0 <= W.kfs[k]["oct"][i] < NLEVELS:
                R.flags |= LBA_BAD_INDEX
                continue
            mine.append((k, i, int(starts[p]) + j))
        per_point.append(mine)
    R.num_fixed = len(R.fixed) + (1 if any(W.kfs[k]["id"] == init_id for k in R.llist) else 0)
    if R.num_fixed < 2:   # :1885-1931
        lower, second, k_lower, k_second = int32(pKF["id"]), int32(pKF["id"]), None, None
        for k in R.llist:
            if k == cur or W.kfs[k]["id"] == init_id:
                continue
            i = int32(W.kfs[k]["id"])
            if i < lower:
                if variant == "hand_down":   # the wrong variant: the old lowest becomes the second
                    second, k_second = lower, k_lower
                lower, k_lower = i, k
            elif i < second:
                second, k_second = i, k
        if k_lower is not None:
            R.fixed.append(k_lower)
            R.llist.remove(k_lower)
            R.num_fixed += 1
            if R.num_fixed < 2 and k_second is not None:
                R.fixed.append(k_second)
                R.llist.remove(k_second)
                R.num_fixed += 1
    # ---- the graph (:1957-2190)
    R.vertices = sorted(set(R.llist) | set(R.fixed), key=lambda k: (W.kfs[k]["id"] & 0xFFFFFFFF, k))
    pose_of = {k: r for r, k in enumerate(R.vertices)}
    for l, mine in enumerate(per_point):
        for k, i, o in mine:
            ur = W.kfs[k]["u_right"][i]
            mono = bool(ur < 0)
            e = np.zeros(1, EDGE_DTYPE)[0]
            e["pose"], e["point"], e["kind"], e["cam"] = pose_of[k], l, EDGE_MONO if mono else EDGE_STEREO, 0
            e["obs"] = (W.kfs[k]["xy"][i][0], W.kfs[k]["xy"][i][1], f32(0) if mono else ur)
            e["inv_sigma2"] = INV_SIGMA2[W.kfs[k]["oct"][i]]
            R.edges.append(e)
            R.edge_rec.append(o)
    return finish_build(W, R, init_id, caps)


def view_n_ordered(view, cur):
    return view["_n_ordered"][cur]


def finish_build(W, R, init_id, caps):
    cap_p, cap_l, cap_e = caps
    R.n_poses, R.n_points, R.n_edges = len(R.vertices), len(R.points), len(R.edges)
    R.edges = np.array(R.edges, EDGE_DTYPE) if R.edges else np.zeros(0, EDGE_DTYPE)
    R.overflow = R.n_poses > cap_p or R.n_points > cap_l or R.n_edges > cap_e
    words = np.zeros(LBA_R_WORDS, np.int32)
    words[[LBA_R_N_POSES_REQUIRED, LBA_R_N_POINTS_REQUIRED, LBA_R_N_EDGES_REQUIRED]] = R.n_poses, R.n_points, R.n_edges
    if R.overflow:
        R.flags |= LBA_OVERFLOW
    else:
        local = set(R.llist)
        R.poses = np.array([pose_from_tcw(W.kfs[k]["R"], W.kfs[k]["t"]) for k in R.vertices], f64).reshape(-1, 7)
        R.hidx, n_free = [], 0
        for k in R.vertices:
            free = k in local and W.kfs[k]["id"] != init_id
            R.hidx.append(n_free if free else -1)
            n_free += free
        R.pose_local = [1 if k in local else 0 for k in R.vertices]
        R.xyz = np.array([W.mps[p]["pos"].astype(f64) for p in R.points], f64).reshape(-1, 3)
        R.lm_start, R.pose_start, R.pose_edges = build_structure(R.edges, R.n_poses, R.n_points)
        n_mono = int((R.edges["kind"] == EDGE_MONO).sum())
        words[[LBA_R_N_LOCAL, LBA_R_N_FIXED, LBA_R_NUM_FIXED_KF, LBA_R_N_POINTS, LBA_R_N_EDGES, LBA_R_N_MONO, LBA_R_N_STEREO]] = \
            len(R.llist), len(R.fixed), R.num_fixed, R.n_points, R.n_edges, n_mono, R.n_edges - n_mono
    words[LBA_R_FLAGS] = R.flags
    R.words = words
    return R


def compare_window(R, win, caps):
    cap_p, cap_l, cap_e = caps
    h = {k: host(v) for k, v in win.items() if k != "work"}
    assert h["result"].tolist() == R.words.tolist(), (h["result"].tolist(), R.words.tolist())
    if R.overflow:                                              # nothing but the result words was written
        for k, a in h.items():
            if k != "result":
                assert (a.view(np.uint8) == FILL).all(), k
        return
    npz, nl, ne = R.n_poses, R.n_points, R.n_edges
    assert (int(h["n_poses"][0]), int(h["n_points"][0]), int(h["n_edges"][0])) == (npz, nl, ne)
    assert h["poses"][:npz].tobytes() == R.poses.tobytes()
    assert h["pose_hidx"].tolist() == R.hidx + [-1] * (cap_p - npz)
    assert h["pose_kf"].tolist() == R.vertices + [-1] * (cap_p - npz)
    assert h["pose_local"].tolist() == R.pose_local + [0] * (cap_p - npz)
    assert h["points"][:nl].tobytes() == R.xyz.tobytes()
    assert h["point_mp"].tolist() == R.points + [-1] * (cap_l - nl)
    assert host(win["edges"], EDGE_DTYPE)[:ne].tobytes() == R.edges.tobytes()
    assert h["edge_rec"][:ne].tolist() == R.edge_rec
    assert h["lm_start"].tobytes() == np.concatenate([R.lm_start, np.full(cap_l - nl, ne, np.int32)]).tobytes()
    assert h["pose_start"].tobytes() == np.concatenate([R.pose_start, np.full(cap_p - npz, ne, np.int32)]).tobytes()
    assert h["pose_edges"][:ne].tobytes() == R.pose_edges.tobytes()


def run_build(L, backend, W, cur, init_id=None, caps=None, csr=None, kf_mp_raw=None, covis_raw=None, use_map=True, variant=None, **damage):
    """the call on the flattened world against the restatement -> (Result, device view, device kfs, window, LocalBA)"""
    init_id = 100 if init_id is None else init_id
    view, kfs, recs = flatten(W, csr, kf_mp_raw, covis_raw, use_map=use_map, **damage)
    rview = None
    if damage:
        rview = dict(view, _n_ordered=kfs["n_ordered"], _cap_conn=kfs["ordered_kf"].shape[1])
    Wr = W
    if not use_map:                                             # d_map = NULL: every key frame is in the one map
        Wr = copy.deepcopy(W)
        for k in Wr.kfs:
            if k is not None:
                k["map"] = 0
    R0 = restate_build(Wr, recs, cur, init_id, (1 << 30,) * 3, kf_mp_raw, covis_raw, variant, rview)
    caps = caps or (max(R0.n_poses, 1) + 2, max(R0.n_points, 1) + 3, max(R0.n_edges, 1) + 5)
    R = restate_build(Wr, recs, cur, init_id, caps, kf_mp_raw, covis_raw, variant, rview)
    dv, dk = upload(view, kfs, backend)
    ba = LocalBA(INV_SIGMA2, SF, CAM, *caps, lib=L)
    win = ba.Window(dv["obs_start"])
    fill(win)
    ba.Build(dv, dk, cur, init_id, win)
    compare_window(R, win, caps)
    return R, dv, dk, win, ba


# ------------------------------------------------------------------------------------------------ the restatement: the apply
def restate_apply(W0, B, chi2, depth, poses, points, use_nobs=True, variant=None):
    """Optimizer.cc:2293-2510 serially on the restated window B with the optimised poses / points"""
    W, R = copy.deepcopy(W0), Result()
    ne = B.n_edges
    order = [e for e in range(ne) if B.edges[e]["kind"] == EDGE_MONO] + [e for e in range(ne) if B.edges[e]["kind"] != EDGE_MONO]
    if variant == "record_order":   # the wrong variant: vToErase in edge order
        order = list(range(ne))
    to_erase = []
    for e in order:
        th = f64(5.991) if B.edges[e]["kind"] == EDGE_MONO else f64(7.815)
        if f64(chi2[e]) > th or not f64(depth[e]) > f64(0.0):
            to_erase.append((B.vertices[B.edges[e]["pose"]], B.points[B.edges[e]["point"]]))
    n_mono = int((B.edges["kind"] == EDGE_MONO).sum())
    R.erased, R.n_mono, R.n_stereo, R.went_bad = to_erase, n_mono, ne - n_mono, []
    R.early = float(len(to_erase)) >= (n_mono + (ne - n_mono)) * 0.5
    R.W = W
    if R.early:
        return R
    ref0 = {p: (W.mps[p]["ref_kf"], W.mps[p]["level"]) for p in B.points}
    touched = set()
    for k, p in to_erase:   # :2390-2401
        m = W.mps[p]
        if m["bad"] or k not in m["obs"]:
            continue
        if not use_nobs and p not in touched:
            m["nObs"] = W.weight_sum(m)
        touched.add(p)
        i = m["obs"][k]
        W.kfs[k]["mp"][i] = None                            # EraseMapPointMatch(pMP) through GetIndexInKeyFrame, whatever the slot holds
        del m["obs"][k]                                     # EraseObservation
        m["nObs"] -= 2 if W.kfs[k]["u_right"][i] >= 0 else 1
        if m["ref_kf"] == k and m["obs"]:
            k2, i2 = W.items_of(m)[0]
            m["ref_kf"], m["level"] = k2, W.kfs[k2]["oct"][i2]
        if m["nObs"] <= 2:                                  # SetBadFlag
            m["bad"] = True
            for k2, i2 in m["obs"].items():
                W.kfs[k2]["mp"][i2] = None
            m["obs"] = {}
            m["ref_kf"], m["level"] = ref0[p]               # (a bad point keeps its d_ref entry)
            R.went_bad.append(p)
    R.went_bad.sort(key=B.points.index)
    R.touched = touched
    for r, k in enumerate(B.vertices):   # :2425-2433
        if B.pose_local[r]:
            kf = W.kfs[k]
            kf["R"], kf["t"] = pose_to_float(poses[r])
            kf["center"] = ow_gemm(kf["R"], kf["t"], variant)
    for l, p in enumerate(B.points):     # :2499-2506
        m = W.mps[p]
        m["pos"] = np.asarray(points[l], f64).astype(f32)
        if not m["bad"] and m["obs"]:
            items = W.items(p)
            m["normal"], m["min_d"], m["max_d"] = normal_and_depth(m["pos"], [W.kfs[k]["center"] for k, _ in items],
                                                                   W.kfs[m["ref_kf"]]["center"], SF[m["level"]], SF[NLEVELS - 1])
    return R


def compare_map(W, view0, dv, dk, out, use_nobs, touched=None):
    """the map as the device holds it against the restated world W"""
    want_v, want_k, _ = flatten(W)
    mp, want_mp = host(dv["mp"], MAP_POINT_DTYPE), want_v["mp"].copy()
    if touched is not None:                                     # ORBM_MP_HAS_OBS is rewritten for the points that lost a record only
        keep = np.array([p not in touched for p in range(len(W.mps))], bool)
        want_mp["flags"][keep] = view0["mp"]["flags"][keep]
    assert mp.tobytes() == want_mp.tobytes()
    assert host(dv["kf_mp"]).tolist() == want_v["kf_mp"].tolist()
    if use_nobs:
        assert host(dk["mp_nobs"]).tolist() == want_k["mp_nobs"].tolist()
    assert host(dk["ref"], REFRESH_POINT_DTYPE).tobytes() == want_k["ref"].tobytes()
    assert host(dk["pose"], FUSENB_POSE_DTYPE).tobytes() == want_k["pose"].tobytes()
    assert host(dk["center"], KEYFRAME_CENTER_DTYPE).tobytes() == want_k["center"].tobytes()
    if out is not None:
        start, obs = host(out["obs_start"]), host(out["obs"], OBSERVATION_DTYPE)
        assert start.tolist() == want_v["obs_start"].tolist()
        assert obs[:int(start[-1])].tobytes() == want_v["obs"].tobytes()


def set_dev(dst, src, backend):
    """src (a host array) into the head of the device array dst"""
    if backend == "emu":
        dst.reshape(-1)[:src.size] = src.reshape(-1)
    else:
        import torch
        dst.view(-1)[:src.size] = torch.from_numpy(np.ascontiguousarray(src).reshape(-1)).to(dst.device)


def run_apply(L, backend, W, cur, chi2, depth, init_id=None, poses=None, points=None, use_nobs=True, variant=None):
    """Build, then Apply with the given chi2 / depth (and poses / points in place of the solver's) against the restatement"""
    B, dv, dk, win, ba = run_build(L, backend, W, cur, init_id)
    view0, kfs0, _ = flatten(W)
    if not use_nobs:
        del dk["mp_nobs"]
    chi2, depth = np.asarray(chi2, f64), np.asarray(depth, f64)
    assert len(chi2) == len(depth) == B.n_edges
    poses = B.poses if poses is None else np.asarray(poses, f64)
    points = B.xyz if points is None else np.asarray(points, f64)
    set_dev(win["chi2"], chi2, backend); set_dev(win["depth"], depth, backend)
    set_dev(win["poses"], poses, backend); set_dev(win["points"], points, backend)
    out = ba.Apply(dv, dk, win)
    R = restate_apply(W, B, chi2, depth, poses, points, use_nobs, variant)
    res = host(out["result"])
    want = np.zeros(LBA_A_WORDS, np.int32)
    want[[LBA_A_FLAGS, LBA_A_N_ERASED, LBA_A_N_WENT_BAD, LBA_A_N_MONO, LBA_A_N_STEREO]] = \
        LBA_EARLY_RETURN if R.early else 0, len(R.erased), len(R.went_bad), R.n_mono, R.n_stereo
    want[LBA_A_N_OBS] = sum(len(m["obs"]) for m in R.W.mps)
    assert res.tolist() == want.tolist(), (res.tolist(), want.tolist())
    assert host(out["erased"])[:len(R.erased)].tolist() == [list(e) for e in R.erased]
    cap_l = ba.caps[1]
    assert host(out["went_bad"]).tolist() == R.went_bad + [-1] * (cap_l - len(R.went_bad))
    compare_map(R.W, view0, dv, dk, out, use_nobs, None if R.early else R.touched)
    if R.early:                                                 # the map as given, bytes
        assert host(dv["mp"], MAP_POINT_DTYPE).tobytes() == view0["mp"].tobytes()
        assert host(dk["pose"], FUSENB_POSE_DTYPE).tobytes() == kfs0["pose"].tobytes()
    return R, B, (dv, dk, out)


# ------------------------------------------------------------------------------------------------ worlds
def rot(rng, scale=0.3):
    from orbhip.lba import _rodrigues
    return _rodrigues(rng.normal(0, scale, 3)).astype(f32)


def random_world(rng, n_kf=7, n_mp=30, n_feat=12, p_bad_kf=0.15, p_bad_mp=0.1, p_stereo=0.5, p_foreign=0.1, n_covis=None):
    kfs = []
    for k in range(n_kf):
        nf = int(rng.integers(max(n_feat - 4, 1), n_feat + 1))
        mp = [int(p) if rng.random() < 0.8 else None for p in rng.integers(0, n_mp, nf)]
        ur = [f32(rng.uniform(0, 700)) if rng.random() < p_stereo else f32(-1) for _ in range(nf)]
        kfs.append(KF(mp, ur, oct=rng.integers(0, NLEVELS, nf).tolist(), xy=[(f32(rng.uniform(0, 752)), f32(rng.uniform(0, 480))) for _ in range(nf)],
                      R=rot(rng), t=rng.normal(0, 2, 3), bad=bool(rng.random() < p_bad_kf), map=int(rng.random() < p_foreign)))
    ids = rng.permutation(n_kf * 3)[:n_kf]
    for k, kf in enumerate(kfs):
        kf["id"] = int(ids[k])
    mps = [MP(rng.normal(0, 3, 3), bad=bool(rng.random() < p_bad_mp), normal=rng.normal(0, 1, 3).astype(f32)) for _ in range(n_mp)]
    W = link(World(kfs, mps, order=rng.permutation(n_kf).tolist()))
    for m in W.mps:
        if m["obs"]:
            k, i = W.items_of(m)[int(rng.integers(0, len(m["obs"])))]
            m["ref_kf"], m["level"] = k, W.kfs[k]["oct"][i]
    cur = int(rng.integers(0, n_kf))
    kfs[cur]["map"] = 0
    for k, kf in enumerate(kfs):
        others = [j for j in range(n_kf) if j != k]
        n = int(rng.integers(0, len(others) + 1)) if n_covis is None else min(n_covis, len(others))
        kf["covis"] = [int(j) for j in rng.permutation(others)[:n]]
    return W, cur


def chain_world(n_kf, fixed_kf=()):
    """key frame k holds points 2k .. 2k+5: neighbours share four points.  Every key frame is covisible with key frame n_kf - 1 but `fixed_kf`"""
    kfs = [KF([2 * k + j for j in range(6)], t=(0.1 * k, 0, 0), id=10 + k) for k in range(n_kf)]
    W = link(World(kfs, [MP((0.1 * p, 0.2, 4.0)) for p in range(2 * n_kf + 4)]))
    kfs[n_kf - 1]["covis"] = [k for k in range(n_kf - 2, -1, -1) if k not in fixed_kf]
    return W, n_kf - 1


# ------------------------------------------------------------------------------------------------ the build: constructed cases
@pytest.mark.parametrize("backend", BACKENDS)
def test_build_hand_computed_world(lib, backend):
    """three key frames, ids 7 < 8 < 9 in slots 2, 0, 1; the current one (slot 1) sees slot 0; slot 2 only shares point 1: fixed"""
    kfs = [KF([0, 1], u_right=[-1, 30.5], oct=[1, 2], xy=[(11, 12), (13, 14)], id=8, t=(1, 0, 0)),
           KF([0, None], u_right=[-1, -1], oct=[0, 0], xy=[(21, 22), (23, 24)], id=9, t=(2, 0, 0)),
           KF([1], u_right=[-1], oct=[3], xy=[(31, 32)], id=7, t=(3, 0, 0))]
    kfs[1]["covis"] = [0]
    W = link(World(kfs, [MP((1, 2, 3)), MP((4, 5, 6))], order=[1, 0, 2]))
    R, *_ = run_build(lib, backend, W, 1, init_id=0)
    # one fixed key frame is fewer than two: the branch moves the lowest local id that is not the current one's (8, slot 0) to the fixed ones
    assert R.llist == [1] and R.points == [0, 1] and R.fixed == [2, 0] and R.vertices == [2, 0, 1] and R.hidx == [-1, -1, 0]
    assert R.num_fixed == 2 and R.pose_local == [0, 0, 1]
    # point 0: records in rank order (slot 1, then slot 0); point 1: slot 0 (stereo), slot 2
    assert R.edges["pose"].tolist() == [2, 1, 1, 0] and R.edges["kind"].tolist() == [EDGE_MONO, EDGE_MONO, EDGE_STEREO, EDGE_MONO]
    assert R.edges["obs"].tolist() == [[21, 22, 0], [11, 12, 0], [13, 14, 30.5], [31, 32, 0]]
    assert R.edges["inv_sigma2"].tolist() == [INV_SIGMA2[0], INV_SIGMA2[1], INV_SIGMA2[2], INV_SIGMA2[3]]


@pytest.mark.parametrize("backend", BACKENDS)
def test_build_bad_covisible_keyframe_and_foreign_map(lib, backend):
    """a bad covisible key frame is marked local (so never fixed), not listed, and takes no edge; a key frame of another map likewise"""
    W, cur = chain_world(6)
    W.kfs[3]["bad"], W.kfs[2]["map"] = True, 5
    R, *_ = run_build(lib, backend, W, cur)
    assert 3 not in R.vertices and 2 not in R.vertices and 3 not in R.llist
    W.kfs[cur]["covis"].remove(3)                               # not covisible: still neither fixed nor an edge
    R, *_ = run_build(lib, backend, W, cur)
    assert 3 not in R.vertices
    run_build(lib, backend, W, cur, use_map=False)              # d_map = NULL: one map, key frame 2 is local again


@pytest.mark.parametrize("backend", BACKENDS)
def test_build_point_occurrences_bad_point_and_null(lib, backend):
    """a point in two key frames and in two features of one is listed once, at its first place; a bad point and a null entry are skipped"""
    kfs = [KF([3, None, 0, 3, 1]), KF([1, 0, 2, 2]), KF([2, 4])]
    kfs[0]["covis"] = [1]
    W = link(World(kfs, [MP(), MP(), MP(), MP(), MP()]))
    W.mps[1]["bad"] = True
    R, *_ = run_build(lib, backend, W, 0)
    assert R.points == [3, 0, 2] and R.fixed == [2]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", ["none_fixed", "one_fixed", "init_local", "two_fixed", "else_if", "no_candidate"])
def test_build_fixed_keyframes_and_the_branch(lib, backend, case):
    if case == "no_candidate":                                  # the current key frame alone: the reference dereferences an uninitialised pointer
        W = link(World([KF([0, 1])], [MP(), MP()]))
        R, *_ = run_build(lib, backend, W, 0, init_id=0)
        assert R.num_fixed == 0 and R.llist == [0] and R.hidx == [0]
        return
    W, cur = chain_world(6, fixed_kf={"none_fixed": (), "one_fixed": (0,), "init_local": (), "two_fixed": (0, 1), "else_if": ()}[case])
    init_id = 12 if case == "init_local" else 0
    if case == "else_if":                                       # list order 15 | 14, 11, 13, 12, 10 -> lowest 10, second 12 (not 11: the else-if)
        for k, i in zip(W.kfs[cur]["covis"], (14, 11, 13, 12, 10)):
            W.kfs[k]["id"] = i
    R, *_ = run_build(lib, backend, W, cur, init_id=init_id)
    # none_fixed: the ids fall along the list (14, 13, .., 10), so every one is a new lowest and the else-if never names a second: one moves
    want = {"none_fixed": 1, "one_fixed": 2, "init_local": 2, "two_fixed": 2, "else_if": 2}[case]
    assert R.num_fixed == want
    if case == "none_fixed":
        assert R.fixed == [0] and 0 not in R.llist and R.hidx[0] == -1
    if case == "init_local":
        assert R.hidx[R.vertices.index(2)] == -1 and R.pose_local[R.vertices.index(2)] == 1 and len(R.fixed) == 1
    if case == "else_if":
        ids = [W.kfs[k]["id"] for k in R.fixed]
        assert ids == [10, 12]
        view, kfs, recs = flatten(W)
        wrong = restate_build(W, recs, cur, init_id, (99, 99, 999), variant="hand_down")
        assert [W.kfs[k]["id"] for k in wrong.fixed] == [10, 11]   # the variant that hands the old lowest down differs: the case discriminates


@pytest.mark.parametrize("backend", BACKENDS)
def test_build_poses_ordered_by_id_not_slot_and_signed_ids(lib, backend):
    W, cur = chain_world(6, fixed_kf=(0,))
    for k, i in enumerate((50, 3, 0xFFFFFFF0, 20, 7, 30)):      # one id above 2^31: unsigned in the pose order, signed in the `< 2` walk
        W.kfs[k]["id"] = i
    R, *_ = run_build(lib, backend, W, cur, init_id=1)
    assert [W.kfs[k]["id"] for k in R.vertices] == sorted(W.kfs[k]["id"] for k in R.vertices) and R.vertices != sorted(R.vertices)
    assert W.kfs[R.fixed[-1]]["id"] == 0xFFFFFFF0               # (int)mnId is -16: the lowest


@pytest.mark.parametrize("backend", BACKENDS)
def test_build_u_right_zero_and_negative_zero_are_stereo(lib, backend):
    kfs = [KF([0, 1, 2], u_right=[f32(-1), f32(0), f32(-0.0)]), KF([0, 1, 2])]
    kfs[0]["covis"] = [1]
    R, *_ = run_build(lib, backend, link(World(kfs, [MP(), MP(), MP()])), 0)
    mine = R.edges[R.edges["pose"] == R.vertices.index(0)]
    assert mine["kind"].tolist() == [EDGE_MONO, EDGE_STEREO, EDGE_STEREO]
    assert mine["obs"][:, 2].tobytes() == np.array([0, 0, -0.0], f32).tobytes()


QUAT_CASES = {"trace": np.eye(3), "x": np.diag([1, -1, -1]), "y": np.diag([-1, 1, -1]), "z": np.diag([-1, -1, 1]),
              "w_negative": np.array([[-0.5, 0.8, 0.3], [-0.6, -0.7, 0.4], [0.5, 0.0, -0.2]])}


@pytest.mark.parametrize("backend", BACKENDS)
def test_build_pose_from_tcw_branches(lib, backend):
    """every quaternion branch of poseFromTcw (positive trace, each diagonal maximum, w < 0 before the sign flip), perturbed off the exact
    matrices so that the roundings matter; bytes against the numpy restatement (compare_window)"""
    rng = np.random.default_rng(5)
    from orbhip.lba import _rodrigues
    names = list(QUAT_CASES)
    kfs = [KF([0, 1], R=(QUAT_CASES[n] @ _rodrigues(rng.normal(0, 0.05, 3)) if n != "w_negative" else QUAT_CASES[n]).astype(f32),
              t=rng.normal(0, 3, 3)) for n in names]
    kfs[0]["covis"] = list(range(1, len(names)))
    R, *_ = run_build(lib, backend, link(World(kfs, [MP(), MP()])), 0)
    m = {n: kfs[i]["R"].astype(f64) for i, n in enumerate(names)}
    assert np.trace(m["trace"]) > 0 and all(np.trace(m[n]) <= 0 for n in ("x", "y", "z", "w_negative"))
    assert np.argmax(np.diag(m["x"])) == 0 and np.argmax(np.diag(m["y"])) == 1 and np.argmax(np.diag(m["z"])) == 2
    i = int(np.argmax(np.diag(m["w_negative"]))); j = (i + 1) % 3; k = (j + 1) % 3
    assert m["w_negative"][k, j] - m["w_negative"][j, k] < 0     # w comes out negative and the quaternion is negated
    assert (R.poses[:, 6] >= 0).all()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n_local_points", [255, 256, 257])
def test_build_sizes_across_a_workgroup(lib, backend, n_local_points):
    """255 / 256 / 257 local points among 300 (n_mp above 256 and no multiple of it), two or three records each: the per-point edge ranges
    straddle the 256-edge chunks of the pose lists"""
    n = n_local_points
    kfs = [KF(list(range(n))), KF(list(range(0, n, 2))), KF(list(range(n - 1, -1, -1))), KF([299, 298])]
    kfs[0]["covis"] = [1]
    W = link(World(kfs, [MP((0.01 * p, 0, 3)) for p in range(300)], order=[2, 0, 3, 1]))
    R, *_ = run_build(lib, backend, W, 0)
    assert R.n_points == n and R.n_edges > 512 and R.fixed == [2]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_build_capacity_full_and_one_over(lib, backend, which):
    W, cur = chain_world(6, fixed_kf=(0,))
    R0, *_ = run_build(lib, backend, W, cur)
    full = [R0.n_poses, R0.n_points, R0.n_edges]
    R, *_ = run_build(lib, backend, W, cur, caps=tuple(full))
    assert not R.overflow
    over = list(full)
    over[which] -= 1
    R, dv, dk, win, ba = run_build(lib, backend, W, cur, caps=tuple(over))   # (compare_window: nothing but the result words was written)
    assert R.overflow and R.words[LBA_R_FLAGS] == LBA_OVERFLOW
    with pytest.raises(OrbHipError) as err:
        ba.check_build(win)
    assert err.value.code == ORB_E_CAPACITY


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", ["list_entry", "kf_mp_entry", "empty_slot", "record_kf", "record_row", "rig_record", "octave", "current", "n_ordered",
                                  "kf_rows", "current_rows", "feature_positions", "csr_range", "csr_negative"])
def test_build_bad_indices_are_flagged_and_absent(lib, backend, case):
    W, cur = chain_world(5, fixed_kf=(0,))
    W.kfs.append(None)                                          # slot 5 is empty
    W.order.append(5); W.rank[5] = 5
    kw, flag = {}, LBA_BAD_INDEX
    if case == "list_entry":
        kw["covis_raw"] = {cur: [3, 77, 5, -2, 2, 1]}
    elif case == "kf_mp_entry":
        kw["kf_mp_raw"] = {(cur, 0): 999, (3, 1): -5}
    elif case == "empty_slot":
        W.mps[9]["valid"] = False
    elif case in ("record_kf", "record_row", "rig_record"):
        view, kfs, recs = flatten(W)
        r = list(recs[8])
        r[1] = {"record_kf": (5, 0, 0), "record_row": (r[1][0], 40, 0), "rig_record": (r[1][0], r[1][1], OBS_RIGHT)}[case]
        kw["csr"] = {8: r}
        flag = LBA_UNSUPPORTED if case == "rig_record" else LBA_BAD_INDEX
    elif case == "octave":
        W.kfs[3]["oct"][2] = NLEVELS
    elif case == "current":
        cur = 5
    n_rows = sum(len(k["mp"]) for k in W.kfs if k is not None)
    if case == "n_ordered":                                     # a count past the row: clamped to the row and flagged
        kw["n_ordered_raw"] = {cur: 1000}
    elif case == "kf_rows":                                     # a covisible key frame whose rows leave the table: a vertex without features,
        kw["kf_rows"] = {3: (n_rows - 2, 6)}                    # and its records cannot be read
    elif case == "current_rows":                                # the current key frame's rows leave the table: nothing is built
        kw["kf_rows"] = {cur: (-1, 6)}
    elif case == "feature_positions":                           # key frame 0 names the whole table as its rows (they overlap the others'): more
        kw["kf_rows"] = {0: (0, n_rows)}                        # feature positions than rows, the positions past the table are dropped
        W.kfs[cur]["covis"] = [0, 3, 2, 1]
    elif case == "csr_range":                                   # point 9's range ends past n_obs (and point 10's begins there)
        kw["obs_start_raw"] = {10: 10 ** 6}
    elif case == "csr_negative":
        kw["obs_start_raw"] = {9: -3}                           # point 9's range begins below 0; point 8's ends there: decreasing
    R, dv, dk, win, ba = run_build(lib, backend, W, cur, **kw)
    assert R.flags == flag
    if case in ("current", "current_rows"):
        assert (R.n_poses, R.n_points, R.n_edges) == (0, 0, 0)
    if case == "kf_rows":
        assert 3 in R.vertices and not (R.edges["pose"] == R.vertices.index(3)).any()
    if case in ("csr_range", "csr_negative"):
        assert 9 in R.points and not (R.edges["point"] == R.points.index(9)).any()
        # the write-back on the same map: flagged, nothing faults, the broken points have no rows, every other point keeps its own
        set_dev(win["chi2"], np.ones(R.n_edges), backend); set_dev(win["depth"], np.ones(R.n_edges), backend)
        out = ba.Apply(dv, dk, win)
        assert host(out["result"])[LBA_A_FLAGS] == LBA_BAD_INDEX
        start, view0 = host(out["obs_start"]), flatten(W)[0]
        broken = (9, 10) if case == "csr_range" else (8, 9)
        for p in range(len(W.mps)):
            assert start[p + 1] - start[p] == (0 if p in broken else view0["obs_start"][p + 1] - view0["obs_start"][p]), p
    with pytest.raises(OrbHipError) as err:
        ba.check_build(win)
    assert err.value.code == ORB_E_INVALID


@pytest.mark.parametrize("backend", BACKENDS)
def test_build_empty_window(lib, backend):
    W = link(World([KF([None, None]), KF([0])], [MP()]))
    R, *_ = run_build(lib, backend, W, 0, init_id=0)
    assert (R.n_poses, R.n_points, R.n_edges) == (1, 0, 0)


def test_invalid_arguments(emu_lib):
    W, cur = chain_world(4)
    view, kfs, _ = flatten(W)
    ba = LocalBA(INV_SIGMA2, SF, CAM, 8, 20, 60, lib=emu_lib)
    for bad in ("pose", "kps"):
        k2 = dict(kfs)
        k2[bad] = kfs[bad][:-1]
        with pytest.raises(OrbHipError) as err:
            ba.Build(view, k2, cur, 0)
        assert err.value.code == ORB_E_INVALID
    with pytest.raises(OrbHipError):
        LocalBA(INV_SIGMA2, SF, CAM, 0, 20, 60, lib=emu_lib)
    with pytest.raises(OrbHipError):
        LocalBA(np.ones(17, f32), np.ones(17, f32), CAM, 8, 20, 60, lib=emu_lib)
    assert emu_lib.orbm_lba_window_build(None, None, 0, 0, None, None, None) == ORB_E_INVALID
    assert emu_lib.orbm_lba_window_apply(None, None, None, None, None, None, None, None) == ORB_E_INVALID
    win = ba.Build(view, kfs, cur, 0)
    with pytest.raises(OrbHipError) as err:                     # the out-CSR can only shrink, but n_obs must fit
        ba.Apply(view, kfs, win, cap_obs_out=len(view["obs"]) - 1)
    assert err.value.code == ORB_E_INVALID
    with pytest.raises(OrbHipError) as err:                     # a workspace of the wrong size is refused by the wrapper
        ba.Build(view, kfs, cur, 0, work=np.zeros(16, np.uint8))
    assert err.value.code == ORB_E_INVALID


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("seed", range(100))
def test_build_random_worlds(lib, backend, seed):
    rng = np.random.default_rng(seed)
    W, cur = random_world(rng, n_kf=int(rng.integers(2, 9)), n_mp=int(rng.integers(5, 40)))
    init_id = W.kfs[int(rng.integers(0, len(W.kfs)))]["id"] if seed % 3 else 9999
    run_build(lib, backend, W, cur, init_id=init_id, use_map=bool(seed % 5))


@pytest.mark.gpu
def test_build_and_apply_graph_replay(hip_lib):
    """both halves captured into one graph and replayed: the same bytes as the eager calls (a fixed number of launches, nothing read on
    the host)"""
    import torch
    rng = np.random.default_rng(3)
    W, cur = random_world(rng, n_kf=7, n_mp=40, p_bad_kf=0.0, p_foreign=0.0)
    view, kfs, recs = flatten(W)
    B = restate_build(W, recs, cur, 9999, (12, 50, 200))
    chi2 = np.where(rng.random(B.n_edges) < 0.1, 9.0, 1.0)
    depth = np.ones(B.n_edges)

    def once(graph):
        dv, dk = upload(view, kfs, "hip")
        ba = LocalBA(INV_SIGMA2, SF, CAM, 12, 50, 200, lib=hip_lib)
        win = ba.Window(dv["obs_start"])
        win["work"] = ba.Workspace(dv, dk)
        set_dev(win["chi2"], chi2, "hip"); set_dev(win["depth"], depth, "hip")
        out = None
        if graph:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                ba.Build(dv, dk, cur, 9999, win)                # warm-up outside the capture (allocations)
                out = ba.Apply(dv, dk, win)
                dv, dk = upload(view, kfs, "hip")
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    ba.Build(dv, dk, cur, 9999, win)
                    ba.Apply(dv, dk, win, out=out)
                g.replay()
            s.synchronize()
        else:
            ba.Build(dv, dk, cur, 9999, win)
            out = ba.Apply(dv, dk, win)
        torch.cuda.synchronize()
        keys = ("poses", "pose_hidx", "points", "edges", "lm_start", "pose_start", "pose_edges", "result")
        return [host(win[k]).tobytes() for k in keys] + [host(dv["mp"]).tobytes(), host(dv["kf_mp"]).tobytes(), host(dk["pose"]).tobytes()] + \
            [host(out[k]).tobytes() for k in ("erased", "went_bad", "obs_start", "obs", "result")]
    assert once(False) == once(True)


# ------------------------------------------------------------------------------------------------ the apply: constructed cases
def apply_world(n_kf=6, stereo=()):
    """chain_world with four records per inner point, the features in `stereo` = {(kf, i)} stereo"""
    W, cur = chain_world(n_kf, fixed_kf=(0,))
    for k, i in stereo:
        W.kfs[k]["u_right"][i] = f32(20)
    for k in range(n_kf):
        W.kfs[k]["R"], W.kfs[k]["t"] = rot(np.random.default_rng(k), 0.2), f32([0.3 * k, 0.1, -0.2])
        W.kfs[k]["center"] = ow_gemm(W.kfs[k]["R"], W.kfs[k]["t"])
    return link(W), cur


def edges_of(B, p):
    l = B.points.index(p)
    return list(range(int(B.lm_start[l]), int(B.lm_start[l + 1])))


@pytest.mark.parametrize("backend", BACKENDS)
def test_apply_thresholds_depth_and_nan(lib, backend):
    """chi2 at 5.991 / 7.815 exactly keeps, one ulp above erases; depth 0.0, -0.0 and NaN erase, the least positive double keeps; a NaN
    chi2 keeps"""
    W, cur = apply_world(8, stereo=[(3, 0), (3, 1), (4, 2)])
    view, kfs, recs = flatten(W)
    B = restate_build(W, recs, cur, 100, (99, 99, 999))
    chi2, depth = np.ones(B.n_edges), np.ones(B.n_edges)
    mono = [e for e in range(B.n_edges) if B.edges[e]["kind"] == EDGE_MONO]
    st = [e for e in range(B.n_edges) if B.edges[e]["kind"] == EDGE_STEREO]
    assert len(st) == 3 and len(mono) > 12
    chi2[mono[0]], chi2[mono[1]] = 5.991, np.nextafter(5.991, 9)
    chi2[st[0]], chi2[st[1]], chi2[st[2]] = 7.815, np.nextafter(7.815, 9), 6.5     # above the mono bound, below the stereo one
    depth[mono[2]], depth[mono[3]], depth[mono[4]], depth[mono[5]] = 0.0, -0.0, 5e-324, np.nan
    chi2[mono[6]] = np.nan
    R, *_ = run_apply(lib, backend, W, cur, chi2, depth)
    want = [mono[1], mono[2], mono[3], mono[5], st[1]]
    assert R.erased == [(B.vertices[B.edges[e]["pose"]], B.points[B.edges[e]["point"]]) for e in want] and not R.early


@pytest.mark.parametrize("backend", BACKENDS)
def test_apply_majority_rule(lib, backend):
    """exactly half the edges outliers: the early return, the map untouched, poses included; one pair below: the write-back"""
    W, cur = apply_world(6)
    view, kfs, recs = flatten(W)
    B = restate_build(W, recs, cur, 100, (99, 99, 999))
    assert B.n_edges % 2 == 0
    poses = B.poses + 1e-3
    poses[:, 3:] /= np.linalg.norm(poses[:, 3:], axis=1)[:, None]
    for n_out, early in ((B.n_edges // 2, True), (B.n_edges // 2 - 1, False)):
        chi2 = np.ones(B.n_edges)
        chi2[:n_out] = 100.0
        R, *_ = run_apply(lib, backend, W, cur, chi2, np.ones(B.n_edges), poses=poses, points=B.xyz + 0.01)
        assert R.early == early and len(R.erased) == n_out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("use_nobs", [True, False])
def test_apply_nobs_landing_on_two_and_three_and_the_erase_order(lib, backend, use_nobs):
    """Point A: 4 mono records, one erased -> nObs 3: stays.  Point B: two erased -> nObs 2: SetBadFlag, its other records die by the point.
    Point C: mono and stereo records, a stereo outlier in an earlier edge than a mono one: mono first leaves another nObs than edge order"""
    W, cur = apply_world(8, stereo=[(5, 0), (5, 1)])             # point 10 = feature 0 of key frame 5, point 11 = feature 1
    view, kfs, recs = flatten(W)
    B = restate_build(W, recs, cur, 100, (99, 99, 999))
    a, b, c = 6, 8, 10
    assert [len(W.mps[p]["obs"]) for p in (a, b, c)] == [3, 3, 3]
    if use_nobs:
        W.mps[a]["nObs"], W.mps[b]["nObs"] = 4, 4                # the counter as the caller tracks it (it may drift from the records)
        W.mps[c]["nObs"] = 5
    chi2 = np.ones(B.n_edges)
    chi2[edges_of(B, a)[0]] = 50
    for e in edges_of(B, b)[:2]:
        chi2[e] = 50
    ec = edges_of(B, c)
    kinds = [int(B.edges[e]["kind"]) for e in ec]
    assert kinds == [EDGE_MONO, EDGE_MONO, EDGE_STEREO]          # key frames 3, 4 (mono features), 5 (stereo)
    chi2[ec[2]] = 50; chi2[ec[0]] = 50                           # the stereo one is first in pointer rank when the order below is reversed
    R, Bd, (dv, dk, out) = run_apply(lib, backend, W, cur, chi2, np.ones(B.n_edges), use_nobs=use_nobs)
    if use_nobs:
        assert not R.W.mps[a]["bad"]
        assert R.W.mps[a]["nObs"] == 3 and R.W.mps[b]["bad"] and R.W.mps[b]["nObs"] == 2 and b in R.went_bad and a not in R.went_bad
        # C: mono first: 5 - 1 = 4 (stays), - 2 = 2: bad with nObs 2.  Stereo first: 5 - 2 = 3, - 1 = 2: the same end here, so pin the order by
        # the erase list instead: the mono pair comes first although its edge is not
        assert R.erased.index((3, c)) < R.erased.index((5, c))
        wrong = restate_apply(W, Bd, chi2, np.ones(B.n_edges), Bd.poses, Bd.xyz, variant="record_order")
        assert wrong.erased != R.erased
    else:
        assert R.W.mps[a]["bad"] and R.W.mps[b]["bad"]           # 3 records of weight 1: one erase lands on 2


@pytest.mark.parametrize("backend", BACKENDS)
def test_apply_mono_then_stereo_leaves_another_nobs(lib, backend):
    """a point with nObs 4 (stereo 2 + mono 1 + mono 1), both the stereo record (an earlier edge) and a mono record outliers.  Mono first:
    4 - 1 = 3, then 3 - 2 = 1 -> bad with nObs 1.  Edge order: 4 - 2 = 2 -> bad at once, the mono pair a no-op: nObs 2"""
    W, cur = apply_world(8, stereo=[(3, 4)])                     # point 10 = feature 4 of key frame 3: the first record in rank order
    view, kfs, recs = flatten(W)
    B = restate_build(W, recs, cur, 100, (99, 99, 999))
    ec = edges_of(B, 10)
    assert [int(B.edges[e]["kind"]) for e in ec] == [EDGE_STEREO, EDGE_MONO, EDGE_MONO] and W.mps[10]["nObs"] == 4
    chi2 = np.ones(B.n_edges)
    chi2[ec[0]], chi2[ec[1]] = 50, 50
    R, Bd, _ = run_apply(lib, backend, W, cur, chi2, np.ones(B.n_edges))
    assert R.W.mps[10]["bad"] and R.W.mps[10]["nObs"] == 1
    wrong = restate_apply(W, Bd, chi2, np.ones(B.n_edges), Bd.poses, Bd.xyz, variant="record_order")
    assert wrong.W.mps[10]["nObs"] == 2                          # the wrong variant differs: the case discriminates


@pytest.mark.parametrize("backend", BACKENDS)
def test_apply_ref_erased_with_and_without_going_bad_and_foreign_slot(lib, backend):
    """the record of mpRefKF dies: a point that stays gets its first surviving record's key frame and octave; one that goes bad keeps its
    entry.  EraseMapPointMatch clears the record's feature even where the slot holds another point.  A bad point's pos is written, its
    normal is not"""
    W, cur = apply_world(8)
    for k in range(8):
        W.kfs[k]["oct"] = [(k + j) % NLEVELS for j in range(6)]
    a, b = 6, 8
    for p in (a, b):
        k, i = W.items(p)[0]
        W.mps[p]["ref_kf"], W.mps[p]["level"] = k, W.kfs[k]["oct"][i]
    W.mps[a]["nObs"] = 5
    ka, ia = W.items(a)[0]
    W.kfs[ka]["mp"][ia] = 15                                    # the slot of a's record holds another point (no record of it there)
    view, kfs, recs = flatten(W)
    B = restate_build(W, recs, cur, 100, (99, 99, 999))
    chi2 = np.ones(B.n_edges)
    chi2[edges_of(B, a)[0]] = 50
    chi2[edges_of(B, b)[0]] = 50
    R, Bd, (dv, dk, out) = run_apply(lib, backend, W, cur, chi2, np.ones(B.n_edges), points=B.xyz + 0.05)
    k2, i2 = R.W.items(a)[0]
    assert (R.W.mps[a]["ref_kf"], R.W.mps[a]["level"]) == (k2, W.kfs[k2]["oct"][i2]) and k2 != ka
    assert R.W.mps[b]["bad"] and R.W.mps[b]["ref_kf"] == W.mps[b]["ref_kf"]
    assert R.W.kfs[ka]["mp"][ia] is None
    mp = host(dv["mp"], MAP_POINT_DTYPE)
    assert mp[b]["pos"].tobytes() != view["mp"][b]["pos"].tobytes() and mp[b]["normal"].tobytes() == view["mp"][b]["normal"].tobytes()
    assert mp[a]["normal"].tobytes() != view["mp"][a]["normal"].tobytes()


@pytest.mark.parametrize("backend", BACKENDS)
def test_apply_init_keyframe_round_trip_and_the_gemm_rule(lib, backend):
    """a local init key frame's pose is rewritten from its unoptimised quaternion: float -> quaternion -> float changes a bit of Rcw.  Ow of
    some key frame differs between the gemm rule and float accumulation (searched with numpy, asserted)"""
    rng = np.random.default_rng(11)
    for _ in range(200):
        W, cur = apply_world(6)
        for k in range(6):
            W.kfs[k]["R"], W.kfs[k]["t"] = rot(rng, 0.7), rng.normal(0, 30, 3).astype(f32)
            W.kfs[k]["center"] = ow_gemm(W.kfs[k]["R"], W.kfs[k]["t"])
        init = W.kfs[3]
        Rf, tf = pose_to_float(pose_from_tcw(init["R"], init["t"]))
        differs = [k for k in range(1, 6) if ow_gemm(*pose_to_float(pose_from_tcw(W.kfs[k]["R"], W.kfs[k]["t"]))).tobytes() !=
                   ow_gemm(*pose_to_float(pose_from_tcw(W.kfs[k]["R"], W.kfs[k]["t"])), variant="float_sum").tobytes()]
        if Rf.tobytes() != init["R"].tobytes() and differs:
            break
    else:
        raise AssertionError("no world found")
    view, kfs, recs = flatten(W)
    B = restate_build(W, recs, cur, init["id"], (99, 99, 999))
    assert B.pose_local[B.vertices.index(3)] == 1 and B.hidx[B.vertices.index(3)] == -1
    R, Bd, (dv, dk, out) = run_apply(lib, backend, W, cur, np.ones(B.n_edges), np.ones(B.n_edges), init_id=init["id"])
    got = host(dk["pose"], FUSENB_POSE_DTYPE)
    assert got[3]["Rcw"].tobytes() != kfs["pose"][3]["Rcw"].tobytes()
    assert got[0]["Rcw"].tobytes() == kfs["pose"][0]["Rcw"].tobytes()     # a fixed key frame is not touched
    wrong = restate_apply(W, Bd, np.ones(B.n_edges), np.ones(B.n_edges), Bd.poses, Bd.xyz, variant="float_sum")
    assert any(wrong.W.kfs[k]["center"].tobytes() != R.W.kfs[k]["center"].tobytes() for k in differs)


@pytest.mark.parametrize("backend", BACKENDS)
def test_apply_sizes_across_a_workgroup(lib, backend):
    n = 257
    kfs = [KF(list(range(n))), KF(list(range(0, n, 2))), KF(list(range(n - 1, -1, -1))), KF(list(range(0, n, 3)), u_right=[5] * len(range(0, n, 3)))]
    kfs[0]["covis"] = [1, 3]
    W = link(World(kfs, [MP((0.01 * p, 0, 3)) for p in range(300)], order=[2, 0, 3, 1]))
    view, k_, recs = flatten(W)
    B = restate_build(W, recs, 0, 100, (9, 999, 9999))
    rng = np.random.default_rng(2)
    chi2 = np.where(rng.random(B.n_edges) < 0.2, 9.0, 1.0)
    R, *_ = run_apply(lib, backend, W, 0, chi2, np.ones(B.n_edges), points=B.xyz + 0.001)
    assert len(R.erased) > 100 and len(R.went_bad) > 20 and not R.early


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("seed", range(100))
def test_apply_random_worlds(lib, backend, seed):
    rng = np.random.default_rng(1000 + seed)
    W, cur = random_world(rng, n_kf=int(rng.integers(3, 9)), n_mp=int(rng.integers(8, 40)), p_bad_kf=0.1)
    view, kfs, recs = flatten(W)
    init_id = W.kfs[int(rng.integers(0, len(W.kfs)))]["id"] if seed % 3 else 9999
    B = restate_build(W, recs, cur, init_id, (99, 99, 9999))
    if seed % 4 == 0:
        for m in W.mps:
            m["nObs"] += int(rng.integers(0, 2))
    chi2 = np.where(rng.random(B.n_edges) < (0.6 if seed % 10 == 0 else 0.15), 9.0, 1.0)
    depth = np.where(rng.random(B.n_edges) < 0.05, -1.0, 1.0)
    poses = B.poses.copy()
    if B.n_poses:
        poses[:, :3] += rng.normal(0, 0.01, (B.n_poses, 3))
        poses[:, 3:] += rng.normal(0, 0.001, (B.n_poses, 4))
        poses[:, 3:] /= np.linalg.norm(poses[:, 3:], axis=1)[:, None]
    run_apply(lib, backend, W, cur, chi2, depth, init_id=init_id, poses=poses, points=B.xyz + rng.normal(0, 0.01, B.xyz.shape),
              use_nobs=bool(seed % 2))


# ------------------------------------------------------------------------------------------------ the chain
def scene_world(seed=0, n_kf=8, n_pts=300, n_feat=60, outliers=0.05):
    """8 key frames on a circle looking at a box of 300 points, 60 features each with real projections (about 140 points end up with the two
    views that constrain them and enter the window), 5 % gross outliers"""
    from orbhip.lba import _rodrigues
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-3, 3, n_pts), rng.uniform(-3, 3, n_pts), rng.uniform(-1.5, 1.5, n_pts)], 1).astype(f32)
    kfs = []
    for k in range(n_kf):      # on a circle of radius 10 looking inward, a quarter radian apart: wide baselines
        a = 0.25 * k
        c = np.array([10 * np.cos(a), 10 * np.sin(a), rng.normal(0, 0.2)])
        z = -c / np.linalg.norm(c) + rng.normal(0, 0.02, 3)
        z /= np.linalg.norm(z)
        x = np.cross(np.array([0, 0, 1.0]), z)
        x /= np.linalg.norm(x)
        Rm = np.stack([x, np.cross(z, x), z]).astype(f32)
        t = (-Rm.astype(f64) @ c).astype(f32)
        Xc = pts.astype(f64) @ Rm.astype(f64).T + t.astype(f64)
        u, v = FX * Xc[:, 0] / Xc[:, 2] + CX, FY * Xc[:, 1] / Xc[:, 2] + CY
        vis = np.nonzero((u > 0) & (u < 752) & (v > 0) & (v < 480))[0]
        sel = vis[(n_feat // 3) * k:(n_feat // 3) * k + n_feat]   # a window that slides by a third: most points have three views
        octv = rng.integers(0, NLEVELS, len(sel))
        noise = rng.normal(0, 1, (len(sel), 3)) * SF[octv][:, None] * 0.7
        gross = rng.random(len(sel)) < outliers
        noise[gross, :2] = rng.normal(0, 30, (int(gross.sum()), 2))
        stereo = rng.random(len(sel)) < 0.4
        ur = np.where(stereo, u[sel] + noise[:, 0] - BF / Xc[sel, 2] + noise[:, 2], -1.0)
        kfs.append(KF([int(p) for p in sel], u_right=ur.astype(f32), oct=octv.tolist(),
                      xy=[(f32(a), f32(b)) for a, b in zip(u[sel] + noise[:, 0], v[sel] + noise[:, 1])], R=Rm, t=t, id=20 + k))
    mps = [MP(pts[p] + rng.normal(0, 0.02, 3).astype(f32)) for p in range(n_pts)]
    W = link(World(kfs, mps, order=rng.permutation(n_kf).tolist()))
    for kf in kfs:             # a point needs two views to be constrained: a feature whose point has one view holds no point
        kf["mp"] = [p if len(W.mps[p]["obs"]) >= 2 else None for p in kf["mp"]]
    link(W)
    for k in range(2, n_kf):   # perturb the free poses off the truth
        W.kfs[k]["t"] = (W.kfs[k]["t"] + rng.normal(0, 0.01, 3)).astype(f32)
        W.kfs[k]["center"] = ow_gemm(W.kfs[k]["R"], W.kfs[k]["t"])
    for m in W.mps:
        if m["obs"]:
            k, i = W.items_of(m)[0]
            m["ref_kf"], m["level"] = k, W.kfs[k]["oct"][i]
    W.kfs[n_kf - 1]["covis"] = list(range(n_kf - 2, 1, -1))     # key frames 0 and 1 are not covisible: fixed
    return W, n_kf - 1


@pytest.mark.parametrize("backend", BACKENDS)
def test_chain_run_against_the_oracle_then_keyframe_culling(lib, backend):
    """Run on device arrays alone, then orbm_cull_keyframes on the out-CSR.  The folded map equals, exactly, the restatement fed with the
    call's own chi2, depth, poses and points; poses and points are held against oracle_lib.lba_optimize(5) then (10) on the host-flattened
    window at the bars of tests/test_lba_parity.py (poses 1e-7, points 1e-6, final chi2 1e-6 relative, the same iteration and trial counts).
    On the oracle's final state no edge lies within 1e-3 relative of its threshold and no depth within 1e-9 of 0 (asserted): the outlier set
    is the oracle's."""
    import oracle_lib as O
    W, cur = scene_world()
    view, kfs, recs = flatten(W)
    B = restate_build(W, recs, cur, 20, (16, 400, 1000))
    assert B.n_poses == 8 and B.n_points > 120 and B.n_edges > 350 and len(B.fixed) == 2 and B.num_fixed == 2
    dv, dk = upload(view, kfs, backend)
    ba = LocalBA(INV_SIGMA2, SF, CAM, 16, 400, 1000, lib=lib)
    res = ba.Run(dv, dk, cur, 20)
    win, out = res["win"], res["out"]
    assert host(win["pose_hidx"])[:8].tolist() == B.hidx and res["num_fixedKF"] == B.num_fixed
    # the oracle on the host-flattened window
    w = dict(poses=B.poses, pose_hidx=np.array(B.hidx, np.int32), points=B.xyz, edges=B.edges)
    huber = (HUBER_MONO, HUBER_STEREO)
    p5, x5, s5 = O.lba_optimize(w, CAM, huber, 5)
    p15, x15, s15 = O.lba_optimize(dict(w, poses=p5, points=x5), CAM, huber, 10)
    for got, want in zip(res["stats"], (s5, s15)):
        assert got[0] == want[0] and got[3] == want[3], (got, want)
        assert abs(got[1] - want[1]) <= 1e-6 * abs(want[1]), (got, want)
    poses, points = host(win["poses"])[:B.n_poses], host(win["points"])[:B.n_points]
    assert np.abs(poses - p15).max() < 1e-7 and np.abs(points - x15).max() < 1e-6
    sys_o = O.lba_build_system(dict(w, poses=p15, points=x15), CAM, huber)
    th = np.where(B.edges["kind"] == EDGE_MONO, 5.991, 7.815)
    assert (np.abs(sys_o["chi2"] - th) > 1e-3 * th).all() and (np.abs(sys_o["depth"]) > 1e-9).all()
    chi2, depth = host(win["chi2"])[:B.n_edges], host(win["depth"])[:B.n_edges]
    assert ((chi2 > th) == (sys_o["chi2"] > th)).all() and ((depth > 0) == (sys_o["depth"] > 0)).all()
    # the folded map against the restatement fed with the call's own numbers
    R = restate_apply(W, B, chi2, depth, poses, points)
    assert not R.early and 5 < len(R.erased) < B.n_edges // 4
    assert res["erased"] == R.erased and res["went_bad"] == R.went_bad
    compare_map(R.W, view, dv, dk, out, True, R.touched)
    # the hand-over: KeyFrameCulling reads the out-CSR and the folded slabs
    from orbhip._abi import CullIn, CullOut, LocalMapView
    from orbhip._lib import ptr, zeros
    from orbhip.matcher import _addr, _nrec
    import ctypes as C
    feat = np.array([(o & 0x3F) | 0x40 | (CULL_FEAT_STEREO if u >= 0 else 0) for kf in W.kfs for o, u in zip(kf["oct"], kf["u_right"])], np.uint8)
    prob = np.zeros(1, CULL_PROBLEM_DTYPE)
    prob[0]["current_kf"], prob[0]["init_kf_id"], prob[0]["n_cand"], prob[0]["n_kf_in_map"] = cur, 20, len(W.kfs[cur]["covis"]), len(W.kfs)
    cand = np.array(W.kfs[cur]["covis"], np.int32)
    d_feat, d_prob, d_cand = to_dev_plain(feat, backend), to_dev(prob, backend), to_dev_plain(cand, backend)
    like = dv["obs_start"]
    n_obs = int(host(out["obs_start"])[-1])
    V = LocalMapView(_addr(dv["mp"]), _addr(out["obs_start"]), _addr(out["obs"]), _addr(dv["kf"]), _addr(dv["kf_mp"]), None, None, None,
                     _nrec(dv["mp"]), n_obs, len(W.kfs), len(feat), 0, 0)
    I = CullIn(_addr(dk["ckf"]), _addr(d_feat), _addr(dk["mp_nobs"]), _addr(d_prob), _addr(d_cand), len(cand), len(cand))
    cap = len(cand)
    co = dict(code=zeros(like, (cap,), np.uint8), nmps=zeros(like, (cap,), np.int32), nred=zeros(like, (cap,), np.int32),
              events=zeros(like, (cap, 12), np.uint8), n_events=zeros(like, (1,), np.int32), flags=zeros(like, (1,), np.int32))
    Oc = CullOut(*[_addr(co[k]) for k in ("code", "nmps", "nred", "events", "n_events", "flags")], cap, 0)
    work = zeros(like, (lib.orbm_cull_workspace_bytes(len(W.kfs), len(W.mps), n_obs, 1),), np.uint8)
    assert lib.orbm_cull_keyframes(C.byref(V), C.byref(I), 1, C.byref(Oc), ptr(work), None) == 0
    assert int(host(co["flags"])[0]) == 0 and (host(co["code"]) != 0).all()
    # nMPs of every candidate is the count over the folded d_kf_mp: the erased matches are gone
    want_nmps = [sum(1 for p in R.W.kfs[k]["mp"] if p is not None and not R.W.mps[p]["bad"]) for k in W.kfs[cur]["covis"]]
    assert host(co["nmps"]).tolist() == want_nmps


# ------------------------------------------------------------------------------------------------ Run's exits, a damaged window, the refusals
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("where", ["before", "between", "no_edges"])
def test_run_exits(lib, backend, where, monkeypatch):
    """the stop flag before the first optimise (the map untouched, nothing applied), raised between the two (bDoMore false: one optimise,
    the write-back still runs), and a window without an edge (the early return without the solver)"""
    W, cur = scene_world()
    if where == "no_edges":
        W = link(World([KF([None, None]), KF([0])], [MP()]))
        cur = 0
    view, kfs, recs = flatten(W)
    dv, dk = upload(view, kfs, backend)
    ba = LocalBA(INV_SIGMA2, SF, CAM, 16, 400, 1000, lib=lib)
    stop = np.array([1 if where == "before" else 0], np.uint8)
    if where == "between":
        first = ba.Optimize

        def optimize(win, iterations, stop_flag=None):
            st = first(win, iterations, stop_flag)
            stop[0] = 1                                         # LocalMapping raises the flag while the first optimise runs its last trial
            return st
        monkeypatch.setattr(ba, "Optimize", optimize)
    res = ba.Run(dv, dk, cur, 20, stop_flag=stop)
    if where == "between":
        assert len(res["stats"]) == 1 and res["out"] is not None and res["erased"] and not res["early_return"]
        B = restate_build(W, recs, cur, 20, (16, 400, 1000))
        R = restate_apply(W, B, host(res["win"]["chi2"])[:B.n_edges], host(res["win"]["depth"])[:B.n_edges],
                          host(res["win"]["poses"])[:B.n_poses], host(res["win"]["points"])[:B.n_points])
        assert res["erased"] == R.erased and res["went_bad"] == R.went_bad
        compare_map(R.W, view, dv, dk, res["out"], True, R.touched)
    else:
        assert res["stats"] == [] and res["out"] is None and res["erased"] == []
        compare_map(W, view, dv, dk, None, True)                # the map as given
        assert res["num_fixedKF"] == restate_build(W, recs, cur, 20, (16, 400, 1000)).num_fixed


@pytest.mark.parametrize("backend", BACKENDS)
def test_apply_on_a_damaged_window(lib, backend):
    """a window whose counts, edge vertices, edge records and pose slots were damaged by hand: flagged ORBM_LBA_BAD_INDEX, the damaged
    edges erase nothing, nothing is read through and nothing faults; the undamaged outlier is still erased"""
    W, cur = apply_world(6)
    B, dv, dk, win, ba = run_build(lib, backend, W, cur)
    ne = B.n_edges
    e = host(win["edges"], EDGE_DTYPE).copy()
    e[0]["pose"], e[1]["point"], e[2]["pose"] = 99, -4, -1
    set_dev(win["edges"], e.view(np.uint8), backend)
    rec = host(win["edge_rec"]).copy()
    rec[3], rec[4] = 10 ** 6, -7                               # records outside their point's range
    set_dev(win["edge_rec"], rec, backend)
    pk = host(win["pose_kf"]).copy()
    local = [i for i in range(B.n_poses) if B.pose_local[i]]
    pk[local[0]] = 77                                           # a local pose whose key-frame slot does not exist
    set_dev(win["pose_kf"], pk, backend)
    set_dev(win["n_poses"], np.array([B.n_poses], np.int32), backend)
    set_dev(win["n_points"], np.array([10 ** 6], np.int32), backend)    # clamped to cap_l
    chi2 = np.ones(ba.caps[2])
    chi2[[0, 1, 2, 3, 4, 6]] = 50.0
    set_dev(win["chi2"], chi2, backend); set_dev(win["depth"], np.ones(ba.caps[2]), backend)
    view0, kfs0, _ = flatten(W)
    out = ba.Apply(dv, dk, win)
    res = host(out["result"])
    assert res[LBA_A_FLAGS] == LBA_BAD_INDEX
    assert res[LBA_A_N_ERASED] == 3                             # edges 3, 4 and 6 reach vToErase; 0, 1, 2 cannot be named
    assert host(out["erased"])[2].tolist() == [B.vertices[B.edges[6]["pose"]], B.points[B.edges[6]["point"]]]
    m6 = W.mps[B.points[B.edges[6]["point"]]]                   # only edge 6's record died, or, where that left nObs <= 2, its point's rows
    lost = len(m6["obs"]) if m6["nObs"] - 1 <= 2 else 1
    assert int(res[LBA_A_N_OBS]) == len(view0["obs"]) - lost and int(res[LBA_A_N_WENT_BAD]) == (1 if lost > 1 else 0)
    assert host(dk["pose"], FUSENB_POSE_DTYPE)[B.vertices[local[0]]].tobytes() == kfs0["pose"][B.vertices[local[0]]].tobytes()


def test_refusals_at_the_c_abi(emu_lib):
    """ORB_E_INVALID of both entry points: misaligned poses / points / workspace / d_mp, nlevels out of range, a null window member, the
    out-CSR arrays being the view's own"""
    import ctypes as C
    from orbhip._abi import LbaApply
    from orbhip._lib import ptr
    W, cur = chain_world(4)
    view, kfs, _ = flatten(W)
    ba = LocalBA(INV_SIGMA2, SF, CAM, 8, 20, 60, lib=emu_lib)
    win = ba.Build(view, kfs, cur, 0)
    V, I = ba._view(view), ba._in(ba._view(view), kfs)
    out = ba.Apply(view, kfs, win)

    def build(V=V, I=I, O=None, work=None):
        O = O if O is not None else ba._window(win)
        return emu_lib.orbm_lba_window_build(C.byref(V), C.byref(I), cur, 0, C.byref(O), ptr(win["work"]) if work is None else work, None)

    def apply(V=V, I=I, **over):
        a = dict(d_mp=view["mp"], d_kf_mp=view["kf_mp"], d_mp_nobs=kfs["mp_nobs"], d_ref=kfs["ref"], d_pose=kfs["pose"], d_center=kfs["center"],
                 d_erased=out["erased"], d_went_bad=out["went_bad"], d_obs_start_out=out["obs_start"], d_obs_out=out["obs"], d_result=out["result"])
        a = {k: (v if isinstance(v, int) else ptr(v).value) for k, v in dict(a, **over).items()}
        A = LbaApply(*[a[k] for k in ("d_mp", "d_kf_mp", "d_mp_nobs", "d_ref", "d_pose", "d_center", "d_erased", "d_went_bad", "d_obs_start_out",
                                      "d_obs_out", "d_result")], len(view["obs"]), 0)
        return emu_lib.orbm_lba_window_apply(C.byref(V), C.byref(I), C.byref(ba._window(win)), ptr(win["chi2"]), ptr(win["depth"]), C.byref(A),
                                             ptr(win["work"]), None)
    assert build() == 0 and apply() == 0
    for member in ("poses", "points"):
        O = ba._window(win)
        setattr(O, member, getattr(O, member) + 8)
        assert build(O=O) == ORB_E_INVALID
    for member in ("pose_hidx", "d_edge_rec", "n_edges", "d_result"):
        O = ba._window(win)
        setattr(O, member, None)
        assert build(O=O) == ORB_E_INVALID
    assert build(work=C.c_void_p(ptr(win["work"]).value + 4)) == ORB_E_INVALID
    for n in (0, 17):
        I2 = ba._in(V, kfs)
        I2.nlevels = n
        assert build(I=I2) == ORB_E_INVALID and apply(I=I2) == ORB_E_INVALID
    V2 = ba._view(view)
    V2.d_mp = V.d_mp + 4
    assert build(V=V2) == ORB_E_INVALID
    assert apply(d_mp=ptr(view["mp"]).value + 4) == ORB_E_INVALID
    assert apply(d_obs_start_out=view["obs_start"]) == ORB_E_INVALID and apply(d_obs_out=view["obs"]) == ORB_E_INVALID
    assert apply(d_went_bad=0) == ORB_E_INVALID and apply(d_pose=0) == ORB_E_INVALID
