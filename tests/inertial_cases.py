"""Constructed inputs for the inertial optimisers (csrc/liba_inertial.hip): windows for liba_optimize / liba_compute_errors and frames for
liba_pose_inertial_kf / liba_pose_inertial_lastframe, each made to enter one branch the generated windows of test_inertial_parity.py never
reach.  Every builder starts from synth_inertial_window / synth_inertial_frame at a small size, edits the arrays, and asserts its own premise
from the CPU oracle's trace (oracle/inertial_oracle.cpp, oib_*_trace), so a case cannot silently stop covering its branch.

Margins.  The kernel and the oracle differ by summation order everywhere and, for the KB8 model, by atan2f against float(atan2) (DESIGN.md
section 2).  Counts (iterations, trials, inliers, masks) are compared exactly, so every decision behind them must not sit on its threshold.
With tol_chi the chi2 tolerance of the camera model (TOL_CHI), a case is accepted only if, in the oracle alone,
  * every accept / reject of an LM trial has |currentChi - tempChi| >= 100 * tol_chi * currentChi,
  * every `(iniChi - currentChi) * 1e3 < iniChi` decision is a factor 2 away from 1e-3,
  * every chi2 a pose-inertial edge is classified with is 100 * tol_chi (relative) away from its threshold.
A case that cannot satisfy them is redesigned (other seed, fewer iterations), never loosened.

Conditioning.  Both sides round every ExpSO3 to float (rule R3 of oracle/inertial_oracle.cpp), so a last-bit difference in a step can move a rotation
entry by one float ulp.  A window far from convergence (the rejected-trial cases: poses 0.8 rad / 5 m off) can amplify that beyond the state and chi2
bars without either side being wrong.  For those cases lm_case runs the oracle a second time with one rotation entry of the first free pose moved by
one float ulp and accepts the case only if iterations and trials are unchanged and the final chi2 and states move by less than a quarter of their
bars.  This, too, is judged from the oracle alone.  The cases near convergence do not need it."""
import numpy as np

import oracle_lib as O
from orbhip._abi import EDGE_CLOSE
from orbhip.inertial import HUBER_INERTIAL, IMU_EDGE_DTYPE, KF_DTYPE, set_cam_poses, synth_inertial_frame, synth_inertial_window, synth_prior
from orbhip.lba import EDGE_DTYPE, HUBER_MONO, HUBER_STEREO, _rodrigues

HUBER = (HUBER_MONO, HUBER_STEREO)
TOL_CHI = {False: 1e-7, True: 1e-4}     # chi2 bar of test_inertial_parity.py: pinhole / KB8
TOL_STATE = {False: 5e-6, True: 2e-5}   # its bar on key-frame states; ten times that on points
_CACHE = {}


def cached(fn, *a):
    """a builder's result, built once per argument list and left unchanged"""
    key = (fn.__name__,) + a
    if key not in _CACHE:
        _CACHE[key] = fn(*a)
    return _CACHE[key]


def is_kb8(w):
    return w["rig"].model[0] == 1


def clone(w):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}


def small(kind, seed, n_opt=3, n_fixed_vis=2, n_pts=40, **kw):
    return synth_inertial_window(seed, n_opt=n_opt, n_fixed_vis=n_fixed_vis, n_pts=n_pts, kind=kind, **kw)


# ---- what the oracle's trace must show ------------------------------------------------------------------------------------------------------
def lm_margins(tr, tol_chi):
    """the two LM margin conditions of the module text, on an oracle trace"""
    for t in tr:
        if t["ok2"]:
            assert abs(t["current_chi"] - t["temp_chi"]) >= 100 * tol_chi * t["current_chi"], ("accept/reject without margin", t)
            assert bool(t["accepted"]) == (t["temp_chi"] < t["current_chi"]), t
    for it in np.unique(tr["it"]):
        t = tr[tr["it"] == it][-1]
        if t["stop"] == O.LM_STOP_RHO_ZERO:
            continue
        gain = (t["ini_chi"] - t["end_chi"]) / t["ini_chi"]
        assert gain >= 2e-3 or gain <= 0.5e-3, ("nBad decision without margin", it, gain)


def well_conditioned(w, lam, its, okf, opts, ost):
    """see "Conditioning" in the module text"""
    fp = free_poses(w)
    if not len(fp):
        return
    w2 = clone(w)
    k = w2["kfs"][fp[0]:fp[0] + 1]
    k["Rwb"][0, 1] = np.nextafter(np.float32(k["Rwb"][0, 1]), np.float32(2.0))
    set_cam_poses(k[0], w["rig"])
    kf2, pts2, st2 = O.inertial_optimize(w2, HUBER, lam, its)
    kb8 = is_kb8(w)
    assert st2[0] == ost[0] and st2[3] == ost[3], ("a one-ulp change of a rotation changes the trial count", ost, st2)
    assert abs(st2[1] - ost[1]) <= 0.25 * TOL_CHI[kb8] * ost[1], ("ill-conditioned: final chi2", abs(st2[1] - ost[1]) / ost[1])
    d = max(np.abs(kf2[f] - okf[f]).max() for f in ("Rwb", "twb", "v", "bg", "ba", "Rcw", "tcw"))
    assert d <= 0.25 * TOL_STATE[kb8] and (not len(opts) or np.abs(pts2 - opts).max() <= 2.5 * TOL_STATE[kb8]), ("ill-conditioned: states", d)


def lm_case(windows, lam, its, branch, premise=None, conditioning=False):
    """-> a case: the windows of one liba_optimize call, the oracle's result and trace of each, margins and `premise(trace, stats, window)` asserted"""
    if isinstance(windows, dict):
        windows = [windows]
    res = []
    for w in windows:
        okf, opts, ost, tr = O.inertial_optimize_trace(w, HUBER, lam, its)
        assert ost[0] >= 0 and len(tr) == ost[3], (branch, ost)
        lm_margins(tr, TOL_CHI[is_kb8(w)])
        if conditioning:
            well_conditioned(w, lam, its, okf, opts, ost)
        if premise is not None:
            premise(tr, ost, w)
        res.append({"kfs": okf, "points": opts, "stats": ost, "trace": tr, "errors": O.inertial_errors(w, HUBER)})
    return {"windows": windows, "lam": lam, "its": its, "oracle": res, "branch": branch}


def reaches(case):
    """which of the rare LM events the oracle's traces of a case contain"""
    out = set()
    for r in case["oracle"]:
        tr = r["trace"]
        if ((tr["ok2"] == 1) & (tr["accepted"] == 0)).any():
            out.add("rejected trial")
        if (tr["ok2"] == 0).any():
            out.add("ok2 == 0")
        if (tr["stop"] == O.LM_STOP_NBAD).any():
            out.add("stop: nBad >= 3")
        if (tr["stop"] == O.LM_STOP_RHO_ZERO).any():
            out.add("stop: rhoLM == 0")
        if len(tr) and tr["stop"][-1] == O.LM_STOP_NONE and r["stats"][0] == case["its"]:
            out.add("stop: iterations cap")
    for w in case["windows"]:
        if 3 in obs_codes(w).values():
            out.add("obsTab code 3")
    return out


def free_poses(w):
    return np.flatnonzero(w["kfs"]["pose_fixed"] == 0)


def obs_codes(w):
    """{(landmark, free key frame): code}: 1 = one edge, 2 = two adjacent edges, 3 = more, or not adjacent (the kernel's obsTab)"""
    fixed = w["kfs"]["pose_fixed"]
    where = {}
    for e, E in enumerate(w["edges"]):
        if not fixed[E["pose"]]:
            where.setdefault((int(E["point"]), int(E["pose"])), []).append(e)
    return {k: (1 if len(v) == 1 else 2 if len(v) == 2 and v[1] == v[0] + 1 else 3) for k, v in where.items()}


# ---- liba_optimize: LM branches -------------------------------------------------------------------------------------------------------------
def perturbed(kind, seed, rot=0.8, trans=5.0, fix_first_pose=False, **kw):
    """the free poses thrown far off (rotation sigma `rot` rad, translation sigma `trans` m): LM trials get rejected"""
    w = small(kind, seed, **kw)
    if fix_first_pose:      # a key frame with a fixed pose and free velocity / biases: only `hi >= 0` marks it for push / pop
        w["kfs"]["pose_fixed"][free_poses(w)[0]] = 1
    rng = np.random.default_rng(seed + 7000)
    for k in free_poses(w):
        w["kfs"][k]["Rwb"] = (w["kfs"][k]["Rwb"].reshape(3, 3) @ _rodrigues(rng.normal(0, rot, 3))).astype(np.float32).astype(np.float64).reshape(-1)
        w["kfs"][k]["twb"] = (w["kfs"][k]["twb"] + rng.normal(0, trans, 3)).astype(np.float32)
        set_cam_poses(w["kfs"][k], w["rig"])
    return w


def _has_reject_then_accept(tr, st, w):
    rej = np.flatnonzero((tr["ok2"] == 1) & (tr["accepted"] == 0))
    assert len(rej) and (tr["accepted"][rej[0]:] == 1).any(), "no rejected trial followed by an accepted one"
    free = w["kfs"][(w["kfs"]["has_imu"] == 1) & (w["kfs"]["imu_fixed"] == 0)]
    assert len(free) >= 2     # key frames whose velocity and biases move in every solved trial, so the pop has something to restore


def case_rejected(kind, seed, its):
    """rejected trials: push / pop of every moving vertex, lambda *= ni; ni *= 2, the qmax loop"""
    return lm_case(perturbed(kind, seed), 1e-9, its, "rejected trials (%s)" % kind, _has_reject_then_accept, conditioning=True)


def case_rejected_fixed_pose_free_imu(seed, its):
    """rejected trials in a window where one key frame has pose_fixed = 1 and free IMU states: its v, bg, ba move in a trial and must come back"""
    def premise(tr, st, w):
        _has_reject_then_accept(tr, st, w)
        k = w["kfs"]
        assert ((k["pose_fixed"] == 1) & (k["has_imu"] == 1) & (k["imu_fixed"] == 0)).sum() == 1
    return lm_case(perturbed("stereo", seed, fix_first_pose=True, n_opt=4), 1e-9, its, "rejected trials, fixed pose with free IMU states", premise, conditioning=True)


def case_cholesky(kind, seed):
    """one inertial edge with a negative definite information matrix: the first trials fail the factorisation (ok2 == false, tempChi = DBL_MAX,
    scale 1e-3, pop) and lambda climbs until it succeeds"""
    w = small(kind, seed)
    w["imu"][0]["info"] = (-1e3 * np.eye(9)).reshape(-1)

    def premise(tr, st, w):
        bad = np.flatnonzero(tr["ok2"] == 0)
        assert len(bad) and (tr["accepted"][bad[-1]:] == 1).any(), "no failed factorisation followed by an accepted trial"
    return lm_case(w, 1e-3, 3, "Cholesky failure (%s)" % kind, premise)


def case_stop_nbad(seed, lam):
    """a huge lambda: every trial is a tiny accepted gradient step, three iterations in a row gain less than 1e-3 -> nBad >= 3 ends the run early"""
    def premise(tr, st, w):
        assert tr["stop"][-1] == O.LM_STOP_NBAD and st[0] == 3 and st[0] < 8, (st, tr["stop"])
    return lm_case(small("stereo", seed), lam, 8, "early stop: nBad >= 3", premise)     # lam = 3e10: gains of 2e-5, 6e-5, 1.8e-4


def case_stop_cap(seed):
    def premise(tr, st, w):
        assert tr["stop"][-1] == O.LM_STOP_NONE and st[0] == 2, st
    return lm_case(small("stereo", seed), 1.0, 2, "stop: iterations cap", premise)


# ---- liba_optimize: obsTab codes ------------------------------------------------------------------------------------------------------------
def camera_major(w):
    """each landmark's edges re-sorted by camera: the two edges of one pose on a two-camera rig are no longer adjacent"""
    w = clone(w)
    e = w["edges"]
    w["edges"] = e[np.lexsort((np.arange(len(e)), e["cam"], e["point"]))]
    return w


def duplicated(w):
    """one edge (the first on a free pose) of every second landmark repeated at the end of the landmark's run"""
    w = clone(w)
    e, fixed, out = w["edges"], w["kfs"]["pose_fixed"], []
    for l in range(len(w["points"])):
        run = e[e["point"] == l]
        out.append(run)
        mine = run[fixed[run["pose"]] == 0]
        if l % 2 == 0 and len(mine):
            out.append(mine[:1])
    w["edges"] = np.concatenate(out)
    return w


def case_obstab(which, seed):
    base = small("fisheye" if which.startswith("kb8") else "stereo", seed, n_pts=30)
    w = {"kb8": lambda: base, "kb8 camera-major": lambda: camera_major(base), "kb8 duplicated": lambda: duplicated(base),
         "pinhole duplicated": lambda: duplicated(base)}[which]()
    codes = set(obs_codes(w).values())
    if which == "kb8":
        assert 2 in codes and 3 not in codes, codes
    elif which == "kb8 camera-major":
        assert 3 in codes and len(w["edges"]) == len(base["edges"]), codes
    else:
        assert 3 in codes and len(w["edges"]) > len(base["edges"]), codes
    assert (np.diff(w["edges"]["point"]) >= 0).all()      # still landmark-major: valid input
    return lm_case(w, 1e-2 if is_kb8(w) else 1.0, 1 if is_kb8(w) else 2, "obsTab: " + which)     # KB8: later iterations gain less than the margin asks


# ---- liba_optimize: vertex configurations ---------------------------------------------------------------------------------------------------
def drop_landmark_edges(w, ls):
    w["edges"] = w["edges"][~np.isin(w["edges"]["point"], ls)]
    return w


def case_vertex(which, seed):
    w = small("stereo", seed, n_opt=4, n_pts=40)
    kf, nk, nl = w["kfs"], len(w["kfs"]), len(w["points"])
    first = int(free_poses(w)[0])
    if which == "no imu":                       # vision only: every key frame has_imu = 0, no inertial edges; DR = 6 * nfp
        kf["has_imu"] = 0; kf["imu_fixed"] = 1
        w["imu"] = w["imu"][:0]
    elif which == "free pose, fixed imu":       # hp >= 0, hi < 0: the inertial edges keep only their pose columns there
        kf["imu_fixed"][first + 1] = 1
    elif which == "fixed pose, free imu":       # hp < 0, hi >= 0: restored by push / pop through `hi` alone
        kf["pose_fixed"][first] = 1
    elif which == "inactive inertial edge":     # an inertial edge between two fixed IMU key frames: reported by imu_chi2, not part of the robust sum
        kf["has_imu"][first - 2] = 1            # the last vision-only fixed key frame becomes a fixed IMU key frame
        E = w["imu"][-1:].copy()
        E["kf1"], E["kf2"] = first - 2, first - 1
        w["imu"] = np.concatenate([w["imu"], E])
        assert kf["pose_fixed"][first - 2] and kf["imu_fixed"][first - 2] and kf["pose_fixed"][first - 1] and kf["imu_fixed"][first - 1]
    elif which == "no visual edges":
        w["edges"] = w["edges"][:0]
    elif which == "free pose without visual edges":    # kfStart[p] == kfStart[p + 1]
        w["edges"] = w["edges"][w["edges"]["pose"] != first + 1]
    elif which == "landmarks without edges":    # leading, two in the middle (the lmStart gap fill over more than one landmark), trailing
        drop_landmark_edges(w, [0, nl // 2, nl // 2 + 1, nl - 1])
        assert not np.isin([0, nl // 2, nl // 2 + 1, nl - 1], w["edges"]["point"]).any() and len(w["edges"]) > 50
    elif which == "landmarks of fixed key frames only":
        e = w["edges"]
        w["edges"] = e[~((e["point"] % 4 == 1) & (kf["pose_fixed"][e["pose"]] == 0))]
        seen = np.unique(w["edges"]["point"][kf["pose_fixed"][w["edges"]["pose"]] == 0])
        assert np.setdiff1d(np.unique(w["edges"]["point"]), seen).size >= 3
    else:
        raise KeyError(which)
    assert nk == len(w["kfs"])
    return lm_case(w, 1.0, 3, "vertex configuration: " + which)


# ---- liba_optimize: counts ------------------------------------------------------------------------------------------------------------------
def case_free_count(n_opt, seed):
    """1, 4, 5 free key frames: poses are dealt to four waves (p = wave; p < nfp; p += 4), Schur tasks likewise"""
    return lm_case(small("mono", seed, n_opt=n_opt, n_pts=36), 1.0, 2, "%d free key frames" % n_opt)


def case_pose_edges(n, seed):
    """one free pose with exactly `n` visual edges (lanes stride over a pose's edges by 64)"""
    w = small("stereo", seed, n_opt=2, n_fixed_vis=1, n_pts=110, max_obs=4)
    k = int(free_poses(w)[-1])
    mine = np.flatnonzero(w["edges"]["pose"] == k)
    assert len(mine) >= n, len(mine)
    keep = np.ones(len(w["edges"]), bool); keep[mine[n:]] = False
    w["edges"] = w["edges"][keep]
    assert (w["edges"]["pose"] == k).sum() == n
    return lm_case(w, 1.0, 2, "a free pose with %d edges" % n)


def case_edge_count(n, seed):
    """exactly `n` visual edges: the counting sort gives thread t the chunk [t * ceil(n / 256), ...)"""
    w = small("mono", seed, n_opt=3, n_pts=70, max_obs=5)
    assert len(w["edges"]) >= n, len(w["edges"])
    w["edges"] = w["edges"][:n]
    return lm_case(w, 1.0, 2, "%d visual edges" % n)


def case_max_free(seed):
    """LIBA_MAX_FREE = 32 free key frames, 480 reduced unknowns (GPU tier only: the emulator needs minutes)"""
    w = small("stereo", seed, n_opt=32, n_fixed_vis=1, n_pts=64, max_obs=8, dt=0.1)
    assert len(free_poses(w)) == 32
    return lm_case(w, 1e-2, 2, "32 free key frames")


# ---- liba_optimize: the Huber kernel of the oldest inertial edge ----------------------------------------------------------------------------
def case_inertial_huber(above, seed):
    w = small("stereo", seed)
    E = w["imu"][-1]
    assert E["huber"] == HUBER_INERTIAL and w["kfs"]["pose_fixed"][E["kf2"]] == 0     # the Huber-carrying edge is active
    w["kfs"]["v"][E["kf2"]] += np.float32(1.0 if above else 0.25)     # the edge's velocity error: chi2 of about 70 / 4.4

    def premise(tr, st, w):
        c = O.inertial_errors(w, HUBER)["imu_chi2"][-1, 0]
        assert (c > 2 * 16.92) if above else (c < 0.5 * 16.92), c
    return lm_case(w, 1.0, 2, "inertial Huber: chi2 %s 16.92" % ("above" if above else "below"), premise)


# ---- liba_optimize: ragged batch, refusals --------------------------------------------------------------------------------------------------
def case_ragged(seed):
    ws = [small("stereo", seed, n_opt=2, n_fixed_vis=1, n_pts=30), small("stereo", seed + 1, n_opt=4, n_fixed_vis=3, n_pts=50),
          small("mono", seed + 2, n_opt=3, n_fixed_vis=2, n_pts=41, max_obs=4)]
    for f in ("kfs", "points", "edges", "imu"):
        assert len({len(w[f]) for w in ws}) == 3, f
    return lm_case(ws, 1.0, 2, "ragged batch with poisoned slack")


REFUSALS = ("point == n_points", "point == -1", "pose == n_kf", "pose == -1", "cam == n_cams", "kf2 without imu", "kf1 == n_kf",
            "more free poses than max_free", "more free poses than max_free, no imu", "every vertex fixed")


def case_refusal(which, seed):
    """-> (case of the valid neighbour, the invalid window, max_free to set or None).  Every index is range-checked by k_liba_optimize before its first
    use as an index, and the window returns before any other access."""
    good = small("stereo", seed, n_opt=3, n_pts=30)
    bad = small("stereo", seed + 1, n_opt=3, n_pts=30)
    e, mid = bad["edges"], len(bad["edges"]) // 2
    max_free = None
    if which == "point == n_points":
        e["point"][-1] = len(bad["points"])
    elif which == "point == -1":            # the first edge: `pe < pp` does not see it (pp = -1 there)
        e["point"][0] = -1
    elif which == "pose == n_kf":
        e["pose"][mid] = len(bad["kfs"])
    elif which == "pose == -1":
        e["pose"][mid] = -1
    elif which == "cam == n_cams":
        e["cam"][mid] = bad["rig"].n_cams
    elif which == "kf2 without imu":
        bad["imu"][-1]["kf2"] = 0
        assert bad["kfs"]["has_imu"][0] == 0
    elif which == "kf1 == n_kf":
        bad["imu"][0]["kf1"] = len(bad["kfs"])
    elif which == "more free poses than max_free":
        bad = small("stereo", seed + 1, n_opt=4, n_pts=30)
        max_free = 3
    elif which == "more free poses than max_free, no imu":      # 4 free poses, 24 unknowns: fits 15 * max_free = 45, not the max_free slots of obsTab
        bad = small("stereo", seed + 1, n_opt=4, n_pts=30)
        bad["kfs"]["has_imu"] = 0; bad["kfs"]["imu_fixed"] = 1
        bad["imu"] = bad["imu"][:0]
        max_free = 3
    elif which == "every vertex fixed":
        bad["kfs"]["pose_fixed"] = 1; bad["kfs"]["imu_fixed"] = 1
    else:
        raise KeyError(which)
    return lm_case(good, 1.0, 2, "refusal: " + which), bad, max_free


# ---- the independent dense step -------------------------------------------------------------------------------------------------------------
def dense_lm_step(w, lam):
    """One LM step from plain linear algebra: the full, unreduced normal equations over [poses | V, G, A | points] from the oracle's per-edge errors
    and Jacobians, (H + lambda I) x = b by numpy.linalg.solve, the update through oib_pose_update and +=.  No Schur complement.
    -> (key frames, points) after the step"""
    kfs, rig, pts, edges, imu = w["kfs"], w["rig"], w["points"], w["edges"], w["imu"]
    nk, nl = len(kfs), len(pts)
    hp, hi, o = np.full(nk, -1), np.full(nk, -1), 0
    for k in range(nk):
        if not kfs[k]["pose_fixed"]:
            hp[k] = o; o += 6
    for k in range(nk):
        if kfs[k]["has_imu"] and not kfs[k]["imu_fixed"]:
            hi[k] = o; o += 9
    lp = o
    n = lp + 3 * nl
    H, b = np.zeros((n, n)), np.zeros(n)

    def add(J, Om, e, rho1, cols):
        keep = cols >= 0
        Jk, ck = J[:, keep], cols[keep]
        H[np.ix_(ck, ck)] += rho1 * Jk.T @ Om @ Jk
        b[ck] += -rho1 * Jk.T @ Om @ e

    def rho1_of(chi, delta):
        return 1.0 if chi <= delta * delta else delta / np.sqrt(chi)
    for i in range(len(edges)):
        E = edges[i:i + 1]
        k, l, D = int(E["pose"][0]), int(E["point"][0]), 3 if E["kind"][0] == 1 else 2
        e, A, B = O.inertial_vis_error(E, kfs[k:k + 1], rig, pts[l], jac=True)
        Om = np.eye(D) * float(E["inv_sigma2"][0])
        J = np.concatenate([B[:D], A[:D]], 1)
        cols = np.concatenate([hp[k] + np.arange(6) if hp[k] >= 0 else np.full(6, -1), lp + 3 * l + np.arange(3)])
        add(J, Om, e[:D], rho1_of(e[:D] @ Om @ e[:D], HUBER[1] if D == 3 else HUBER[0]), cols)
    for i in range(len(imu)):
        E = imu[i:i + 1]
        k1, k2 = int(E["kf1"][0]), int(E["kf2"][0])
        if hp[k1] < 0 and hi[k1] < 0 and hp[k2] < 0 and hi[k2] < 0:
            continue
        J = O.inertial_imu_jacobian(E, kfs[k1:k1 + 1], kfs[k2:k2 + 1])
        e = O.inertial_imu_error(E, kfs[k1:k1 + 1], kfs[k2:k2 + 1], rig)
        Om = E["info"][0].reshape(9, 9)
        cols = np.concatenate([hp[k1] + np.arange(6) if hp[k1] >= 0 else np.full(6, -1), hi[k1] + np.arange(9) if hi[k1] >= 0 else np.full(9, -1),
                               hp[k2] + np.arange(6) if hp[k2] >= 0 else np.full(6, -1), hi[k2] + np.arange(3) if hi[k2] >= 0 else np.full(3, -1)])
        chi = e @ Om @ e
        add(J, Om, e, rho1_of(chi, E["huber"][0]) if E["huber"][0] > 0 else 1.0, cols)
        for off, fld, info in ((3, "bg", "info_g"), (6, "ba", "info_a")):      # EdgeGyroRW / EdgeAccRW: e = b2 - b1, J = [-I, I]
            J2 = np.concatenate([-np.eye(3), np.eye(3)], 1)
            cols = np.concatenate([hi[k1] + off + np.arange(3) if hi[k1] >= 0 else np.full(3, -1), hi[k2] + off + np.arange(3) if hi[k2] >= 0 else np.full(3, -1)])
            add(J2, E[info][0].reshape(3, 3), kfs[k2][fld] - kfs[k1][fld], 1.0, cols)
    # The random-walk information matrices of the generator are not exactly symmetric, so J^T Omega J is not either.  g2o computes the block of a
    # vertex pair once, for (earlier vertex, later vertex), and its transpose stands below the diagonal; of a vertex's own block the factorisation
    # reads the lower triangle.  That is the matrix solved here.
    blk = np.concatenate([np.repeat(np.arange(lp // 3), 3), lp // 3 + np.repeat(np.arange(nl), 3)])
    blk[:6 * int((hp >= 0).sum())] = np.repeat(np.arange(int((hp >= 0).sum())), 6)
    own = blk[:, None] == blk[None, :]
    H = np.where(own, np.tril(H) + np.tril(H, -1).T, np.triu(H) + np.triu(H, 1).T)
    x = np.linalg.solve(H + lam * np.eye(n), b)
    out, opts = kfs.copy(), pts.copy()
    for k in range(nk):
        if hp[k] >= 0:
            out[k:k + 1] = O.inertial_pose_update(out[k:k + 1], rig, x[hp[k]:hp[k] + 6])
        if hi[k] >= 0:
            out[k]["v"] += x[hi[k]:hi[k] + 3]; out[k]["bg"] += x[hi[k] + 3:hi[k] + 6]; out[k]["ba"] += x[hi[k] + 6:hi[k] + 9]
    return out, opts + x[lp:].reshape(nl, 3)


def case_dense(kind, seed):
    """3 key frames (2 free), 12 landmarks, one iteration whose first trial is accepted"""
    w = small(kind, seed, n_opt=2, n_fixed_vis=0, n_pts=12)
    assert len(w["kfs"]) == 3

    def premise(tr, st, w):
        assert len(tr) == 1 and tr["accepted"][0] == 1 and tr["ok2"][0] == 1, tr
    c = lm_case(w, 1e-2 if kind == "fisheye" else 1.0, 1, "dense step (%s)" % kind, premise)
    c["dense"] = dense_lm_step(w, c["lam"])
    return c


# ---- liba_pose_inertial_kf / liba_pose_inertial_lastframe -----------------------------------------------------------------------------------
CHI2_MONO_KF, CHI2_MONO_LF = (12.0, 7.5, 5.991, 5.991), (5.991,) * 4
CHI2_STEREO = (15.6, 9.8, 7.815, 7.815)


def frame(kind, seed, n_pts, n_edges=None, **kw):
    f = synth_inertial_frame(seed, n_pts, kind, **kw)
    if n_edges is not None:
        assert len(f["edges"]) >= n_edges, (len(f["edges"]), n_edges)
        f["edges"] = f["edges"][:n_edges].copy()
    return f


def run_pose_oracle(f, lastframe, rec_init):
    if lastframe:
        fr, pv, outl, H, n, tr = O.pose_inertial_lastframe_trace(f["frame"], f["keyframe"], f["rig"], f["edges"], f["imu"], f["prior"], rec_init)
        return {"frame": fr, "prev": pv, "outlier": outl, "H": H, "n_good": n, "trace": tr}
    fr, outl, H, n, tr = O.pose_inertial_kf_trace(f["frame"], f["keyframe"], f["rig"], f["edges"], f["imu"], rec_init)
    return {"frame": fr, "prev": None, "outlier": outl, "H": H, "n_good": n, "trace": tr}


def pose_margins(f, r, lastframe):
    """every chi2 an edge was classified with is 100 * tol_chi (relative) away from its threshold, in every round and in the recovery pass"""
    tr, e = r["trace"], f["edges"]
    tol = 100 * TOL_CHI[f["rig"].model[0] == 1]
    stereo, close = (e["kind"] & 0xFF) == 1, (e["kind"] & EDGE_CLOSE) != 0
    mono = CHI2_MONO_LF if lastframe else CHI2_MONO_KF
    for it in range(tr["rounds"]):
        th = np.where(stereo, CHI2_STEREO[it], np.where(close, np.float32(1.5) * np.float32(mono[it]), mono[it]))
        c = tr["chi2"][it]
        assert np.isfinite(c).all() and (np.abs(c - th) >= tol * th).all(), ("classification without margin", it, np.abs(c / th - 1).min())
    if tr["recovery"]:
        th = np.where(stereo, 24.0, 18.0)
        assert (np.abs(tr["chi2_recovery"] - th) >= tol * th).all(), "recovery without margin"


def pose_case(frames, lastframe, rec_init, branch, premise=None):
    """-> a case: the frames of one liba_pose_inertial_* call with the oracle's result and trace of each"""
    res = []
    for i, f in enumerate(frames):
        if lastframe and "prior" not in f:
            f["prior"] = synth_prior(f["keyframe"][0], i)
        r = run_pose_oracle(f, lastframe, rec_init)
        pose_margins(f, r, lastframe)
        res.append(r)
    if premise is not None:
        premise(frames, res)
    return {"frames": frames, "lastframe": lastframe, "rec_init": rec_init, "oracle": res, "branch": branch}


EDGE_COUNTS = (0, 5, 6, 7, 63, 64, 65, 129)


EDGE_COUNT_KINDS = ("mono", "stereo", "mono", "stereo", "fisheye", "stereo", "mono", "stereo")


def pose_frame_ok(f, lastframe, rec_init=False):
    """does this frame alone satisfy the classification margins? (the seed searches use it)"""
    try:
        pose_case([dict(f)], lastframe, rec_init, "")
        return True
    except AssertionError:
        return False


def case_edge_counts(lastframe, seeds):
    """n_edges 0, 5, 6, 7 (both early-exit thresholds: ne + 3 < 10, ne + 4 < 10), 63, 64, 65, 129 (the lane-stride loops at 64)"""
    fs = [frame(k, s, 200, n) for s, k, n in zip(seeds, EDGE_COUNT_KINDS, EDGE_COUNTS)]

    def premise(frames, res):
        rounds = [r["trace"]["rounds"] for r in res]
        want = [1 if n + (4 if lastframe else 3) < 10 else 4 for n in EDGE_COUNTS]
        assert rounds == want, (rounds, want)
    return pose_case(fs, lastframe, False, "edge counts %s" % (EDGE_COUNTS,), premise)


def inliers_after_round4(f, lastframe):
    f = dict(f)
    if lastframe and "prior" not in f:
        f["prior"] = synth_prior(f["keyframe"][0], 0)
    r = run_pose_oracle(f, lastframe, True)      # rec_init: the masks are those of round 4
    return len(f["edges"]) - int(r["outlier"].sum())


def frame_with_inliers(kind, seed, want, lastframe):
    """the frame's edge list truncated until the oracle counts exactly `want` inliers after round 4"""
    f = frame(kind, seed, 120)
    for n in range(len(f["edges"]), 9, -1):
        g = dict(f); g["edges"] = f["edges"][:n].copy()
        if inliers_after_round4(g, lastframe) == want:
            if lastframe:
                g["prior"] = synth_prior(g["keyframe"][0], 0)
            return g
    return None


RECOVERY_KINDS = (("mono", 29), ("stereo", 30), ("stereo", 29), ("mono", 30))


def case_recovery(lastframe, rec_init, seeds):
    """29 and 30 inliers after round 4: the recovery pass (chi2 < 18 / 24 re-admits) runs for `nInliers < 30 && !bRecInit` only"""
    fs = [frame_with_inliers(k, s, n, lastframe) for s, (k, n) in zip(seeds, RECOVERY_KINDS)]
    assert all(f is not None for f in fs)

    def premise(frames, res):
        assert [r["trace"]["recovery"] for r in res] == [not rec_init, False, not rec_init, False]
        if not rec_init:      # the pass changed something: an edge classified out in round 4 is back
            assert any((np.nan_to_num(r["trace"]["chi2_recovery"], nan=1e9) < 18).sum() > 29 for r in res if r["trace"]["recovery"])
    return pose_case(fs, lastframe, rec_init, "29 / 30 inliers, rec_init %d" % rec_init, premise)


def behind_frame(seed, lastframe):
    """three well-fitting mono edges mirrored through the camera centre: the same image point at negative depth"""
    f = frame("mono", seed, 80)
    g = dict(f)
    if lastframe:
        g["prior"] = synth_prior(f["keyframe"][0], 0)
    idx = np.argsort(run_pose_oracle(g, lastframe, True)["trace"]["chi2"][3])[:3]
    F = f["frame"][0]
    Rcw, tcw = F["Rcw"][0].reshape(3, 3), F["tcw"][0]
    for i in idx:
        Xc = Rcw @ f["edges"]["xw"][i].astype(np.float64) + tcw
        f["edges"]["xw"][i] = (Rcw.T @ (-Xc - tcw)).astype(np.float32)
        f["edges"]["kind"][i] |= EDGE_CLOSE
    f["behind"] = idx
    if lastframe:
        f["prior"] = g["prior"]
    return f


def case_special_edges(lastframe, seeds):
    """points behind the camera (!depthPositive); mono edges with and without bClose between each round's two thresholds; a frame whose reprojection
    edges are all outliers after round 1 (the system is inertial-only from then on); an edge that is out in round 1 and in again in round 2"""
    behind = behind_frame(seeds[0], lastframe)
    idx = behind["behind"]
    closebit = frame("mono", seeds[1], 90, outliers=0.0)
    e = closebit["edges"]
    e["kind"] = 0
    e["kind"][::2] |= EDGE_CLOSE
    rng = np.random.default_rng(seeds[1])
    sig = 1.0 / np.sqrt(e["inv_sigma2"])
    for j, i in enumerate(range(10, 34)):            # chi2 of about 6.5 ... 16: between chi2Mono and 1.5 * chi2Mono of the rounds
        a = rng.uniform(0, 2 * np.pi)
        e["obs"][i, :2] += (np.sqrt(6.5 + 0.4 * j) * sig[i] * np.array([np.cos(a), np.sin(a)])).astype(np.float32)
    allout = frame("stereo", seeds[2], 40)
    allout["edges"]["obs"][:, 0] += 40.0; allout["edges"]["obs"][:, 1] -= 30.0
    back = frame("stereo", seeds[3], 60)

    def premise(frames, res):
        t0, t1, t2, t3 = [r["trace"] for r in res]
        assert res[0]["outlier"][idx].all() and (t0["chi2"][3][idx] < 5.991).all(), t0["chi2"][:, idx]      # rejected by !depthPositive alone
        m = t1["chi2"][0][10:34]
        assert ((m > 5.991) & (m < 1.5 * 12)).sum() >= 8
        cl = (frames[1]["edges"]["kind"] & EDGE_CLOSE) != 0
        assert res[1]["outlier"][cl].any() and (~res[1]["outlier"][cl].astype(bool)).any() and res[1]["outlier"][~cl].any()
        assert res[2]["outlier"].all() and res[2]["n_good"] == 0 and np.isfinite(t2["chi2"][:t2["rounds"]]).all()
        assert out_then_in(res[3:], frames[3:], lastframe) >= 1, "no edge is classified out and later in again"
    return pose_case([behind, closebit, allout, back], lastframe, True, "special edges", premise)


def out_then_in(res, frames, lastframe):
    """number of edges classified out in one round and in again in a later one (the `outl[e]` re-evaluation at the current state)"""
    n = 0
    mono = CHI2_MONO_LF if lastframe else CHI2_MONO_KF
    for f, r in zip(frames, res):
        e, tr = f["edges"], r["trace"]
        stereo, close = (e["kind"] & 0xFF) == 1, (e["kind"] & EDGE_CLOSE) != 0
        bad = []
        for it in range(tr["rounds"]):
            th = np.where(stereo, CHI2_STEREO[it], np.where(close, np.float32(1.5) * np.float32(mono[it]), mono[it]))
            bad.append(tr["chi2"][it] > th)
        for it in range(1, len(bad)):
            n += int((bad[it - 1] & ~bad[it]).sum())
    return n


def case_prior(seed):
    """LastFrame: a prior whose chi2 exceeds 25 at every step (Huber weight below 1) beside one that stays below"""
    far, near = frame("stereo", seed, 80), frame("stereo", seed + 1, 80)
    far["prior"] = synth_prior(far["keyframe"][0], 1)
    far["prior"]["twb"] += 0.5
    near["prior"] = synth_prior(near["keyframe"][0], 2)

    def premise(frames, res):
        assert res[0]["trace"]["prior_chi2_min"] > 50 and res[1]["trace"]["prior_chi2_max"] < 12.5, (res[0]["trace"]["prior_chi2_min"], res[1]["trace"]["prior_chi2_max"])
        assert all((r["trace"]["gn_steps"] == 10).all() for r in res)
    return pose_case([far, near], True, False, "prior Huber above / below 25", premise)


def case_dropped_sv(seed):
    """LastFrame: zero info_g and a prior without a gyro-bias block: the gyro-bias diagonal of the system is exactly 0, Gauss-Newton's factorisation
    stops at once, and H_pp has three singular values of exactly 0 for pinvJacobi to drop"""
    f = frame("stereo", seed, 80)
    f["imu"] = f["imu"].copy()
    for fld in ("info_g", "JRg", "JVg", "JPg"):      # neither the random walk nor the preintegration ties the gyro biases down
        f["imu"][fld] = 0.0
    pr = synth_prior(f["keyframe"][0], 3)
    H = pr["H"][0].reshape(15, 15).copy()
    H[9:12, :] = 0.0; H[:, 9:12] = 0.0
    pr["H"][0] = H.reshape(-1)
    f["prior"] = pr

    def premise(frames, res):
        tr = res[0]["trace"]
        sv = tr["sv"]
        assert tr["sv_dropped"] >= 1 and (sv[sv > 1e-6] >= 1e-3).all() and (sv[sv <= 1e-6] <= 1e-9).all(), sv
    return pose_case([f], True, False, "dropped singular value", premise)


# ---- poison for the slack of batched slabs --------------------------------------------------------------------------------------------------
def poison_slab(i, a, windows):
    """in place, slab i of a batch (0 key frames, 1 points, 2 visual edges, 3 inertial edges; records as [B, bytes] uint8): NaN coordinates, 1e30
    weights, pose_fixed = 0 behind each window's count; every index stays in range (0)"""
    B = len(windows)
    n = [len(w[("kfs", "points", "edges", "imu")[i]]) for w in windows]
    if i == 0:
        kfs = a.view(KF_DTYPE).reshape(B, -1)
        for b in range(B):
            k = kfs[b, n[b]:]
            for f in ("Rwb", "twb", "Rcw", "tcw", "v", "bg", "ba"):
                k[f] = np.nan
            k["pose_fixed"] = 0; k["has_imu"] = 1; k["imu_fixed"] = 0
    elif i == 1:
        assert a.dtype == np.float64 and a.shape[0] == B and a.shape[2] == 3
        for b in range(B):
            a[b, n[b]:] = np.nan
    elif i == 2:
        edges = a.view(EDGE_DTYPE).reshape(B, -1)
        for b in range(B):
            e = edges[b, n[b]:]
            e["pose"] = 0; e["point"] = 0; e["cam"] = 0; e["kind"] = 1; e["obs"] = np.nan; e["inv_sigma2"] = 1e30
    else:
        imu = a.view(IMU_EDGE_DTYPE).reshape(B, -1)
        for b in range(B):
            r = imu[b, n[b]:]
            for f in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "b", "dT"):
                r[f] = np.nan
            r["kf1"] = 0; r["kf2"] = 0; r["huber"] = 0.0; r["info"] = 1e30; r["info_g"] = 1e30; r["info_a"] = 1e30


def poison_pose_edges(edges, n):
    for b in range(edges.shape[0]):
        e = edges[b, n[b]:]
        e["xw"] = np.nan; e["obs"] = np.nan; e["inv_sigma2"] = 1e30; e["kind"] = 1; e["cam"] = 0
