"""The inertial optimisers (k_liba_optimize, k_liba_errors, k_pose_inertial) on the constructed cases of tests/inertial_cases.py: rejected LM trials,
failed factorisations, early stops, every obsTab code, vertex configurations, counts at the wave / lane / chunk sizes, ragged batches with poison in
the slack, refused windows, and the classification edges of the two pose optimisations.

Each builder has already asserted, from the CPU oracle's trace alone, that its case enters the branch it names and that every decision in it has
margin (inertial_cases.py, "Margins"); here the kernel is compared with the oracle.  stats[0] (iterations), stats[3] (LM trials), outlier masks and
n_good are compared exactly; states and chi2 with the bars test_inertial_parity.py uses and explains (5e-6 pinhole / 2e-5 KB8 on key-frame states, ten
times that on points, 1e-7 / 1e-4 on chi2 and on the final lambda).  The largest deviation seen per backend is printed when the module ends (-s).

Set INERTIAL_CASES_ONLY=1 to stop after the builders: the premises and margins then run without any kernel.

What the file catches.  Each of these one-line changes to csrc/liba_inertial.hip, applied to a scratch copy and run on the emulated build, fails the
named test (first failure, assertion):
   1 pop skips key frames with only hi >= 0       test_rejected_trials_restore_a_fixed_pose_with_free_imu_states   stats[0] / stats[3] (100 trials, lambda inf)
   2 pop does not restore the points              test_rejected_trials_restore_every_vertex[mono]                  final chi2 (0.2 relative)
   3 failed Cholesky taken as ok2 = true          test_failed_factorisation_raises_lambda[stereo]                  stats[3] (16 trials, not 12)
   4 `pose != kj` filter of code 3 dropped        test_obstab_codes[kb8 camera-major]                              stats[3] (7 trials, not 1)
   5 adjacency test always yields code 2          test_obstab_codes[kb8 camera-major]                              final chi2 (7e-4 relative)
   6 imu_active ignores hi                        test_vertex_configurations (fixed pose, free imu)                robust_chi2_sum (5e-5 relative)
   7 random-walk terms dropped from robust_chi    test_rejected_trials_restore_every_vertex[mono]                  robust_chi2_sum (5e-7 relative, bar 1e-9)
   8 lmStart gap fill reduced to l == pe          test_vertex_configurations (landmarks without edges)             final chi2 (3e-2 relative)
   9 trailing lmStart fill dropped                test_rejected_trials_restore_every_vertex[mono]                  final chi2 (8e-4 relative)
  10 early exit `ne + 3` becomes `ne`             test_pose_inertial_edge_counts[kf] (7 edges)                     frame states (2e-3)
  11 recovery thresholds 18 / 24 swapped          test_pose_inertial_recovery_at_29_and_30_inliers[kf-rec0]        n_good (36, not 37)
  12 `if (outl[e]) chiLast[e] = chi2` dropped     test_pose_inertial_edge_counts[lastframe] (129 edges)            outlier mask (edges 68, 114)
  13 `sqrt(s2) > 1e-6` cut dropped                test_lastframe_marginalisation_drops_zero_singular_values        H is not finite
  14 final Hessian loop strides by 32             test_pose_inertial_edge_counts[kf] (63 edges)                    H (0.5 relative)
  15 `nInliers < 30` becomes `<= 30`              test_pose_inertial_recovery_at_29_and_30_inliers[kf-rec0]        n_good (38, not 30)"""
import os

import numpy as np
import pytest

import inertial_cases as K
import oracle_lib as O
from devarrays import BACKENDS, lib, to_dev_plain, to_host  # noqa: F401
from orbhip.inertial import InertialWindows, pose_inertial_optimization_last_frame, pose_inertial_optimization_last_keyframe
from orbhip.lba import POSE_EDGE_DTYPE

CASES_ONLY = bool(os.environ.get("INERTIAL_CASES_ONLY"))
STATE_FIELDS = ("Rwb", "twb", "v", "bg", "ba", "Rcw", "tcw")
DEV = {}     # backend -> quantity -> (largest deviation seen, its bar)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for backend in sorted(DEV):
        print("\nlargest deviations from the oracle, backend %s:" % backend)
        for q in sorted(DEV[backend]):
            print("  %-34s %.3e   (bar %.1e)" % ((q,) + DEV[backend][q]))


def within(backend, what, dev, bar, msg=()):
    """assert dev <= bar, remembering the largest deviation per backend and quantity"""
    dev = float(dev)
    cur = DEV.setdefault(backend, {}).get(what, (0.0, bar))
    DEV[backend][what] = (max(cur[0], dev) if dev == dev else float("nan"), bar)
    assert dev <= bar, (what, dev, bar) + tuple(msg)


# ---- liba_optimize / liba_compute_errors ------------------------------------------------------------------------------------------------------
class PoisoningUploader:
    """The `to_dev` of InertialWindows, which uploads the key-frame, point, edge and inertial-edge slabs first and in that order: before a slab
    leaves the host, the slack behind each window's count is filled with NaN coordinates, 1e30 weights and free vertices (every index in range).
    A kernel that reads the slack shows a mismatch, not an out-of-bounds access."""

    def __init__(self, backend, windows):
        self.backend, self.ws, self.i = backend, windows, 0

    def __call__(self, a):
        if self.i < 4:
            K.poison_slab(self.i, a, self.ws)
        self.i += 1
        return to_dev_plain(a, self.backend)


def make_windows(lib, backend, windows, poison):
    return InertialWindows(windows, PoisoningUploader(backend, windows) if poison else (lambda a: to_dev_plain(a, backend)), lib=lib, huber=K.HUBER)


def run_windows(lib, backend, windows, lam, its, poison=True, max_free=None, errors=True):
    IW = make_windows(lib, backend, windows, poison)
    if max_free is not None:
        IW.prob.max_free = max_free      # before the first optimize(): the workspace is sized from the lowered value
    err = {k: to_host(v) for k, v in IW.compute_errors().items()} if errors else None
    stats = to_host(IW.optimize(lam, its))
    return stats, IW.keyframes(), IW.points(), err


def check_errors(backend, b, w, o, err):
    ne, ni, kb8 = len(w["edges"]), len(w["imu"]), K.is_kb8(w)
    tol = 2e-3 if kb8 else 1e-9      # KB8: float(atan2(double)) vs atan2f, DESIGN.md section 2 (1 float ulp of theta ~ 2e-5 px)
    tag = " (KB8)" if kb8 else " (pinhole)"
    if ne:
        within(backend, "vis_chi2 / max" + tag, np.abs(err["vis_chi2"][b, :ne] - o["vis_chi2"]).max() / max(1.0, o["vis_chi2"].max()), tol, (b,))
        assert np.array_equal(err["vis_depth_pos"][b, :ne], o["vis_depth_pos"]), b
    if ni:
        within(backend, "imu_chi2 / max", np.abs(err["imu_chi2"][b, :ni] - o["imu_chi2"]).max() / max(1.0, o["imu_chi2"].max()), 1e-9, (b,))
    within(backend, "robust_chi2_sum, relative" + tag, abs(err["robust_chi2_sum"][b] - o["robust_chi2_sum"]) / o["robust_chi2_sum"], tol, (b,))


def check_window(backend, b, w, o, stats, kf, pts):
    nk, nl, kb8 = len(w["kfs"]), len(w["points"]), K.is_kb8(w)
    ost, tag = o["stats"], " (KB8)" if kb8 else " (pinhole)"
    assert stats[b, 0] == ost[0] and stats[b, 3] == ost[3], (b, stats[b], ost)
    tc, ts = K.TOL_CHI[kb8], K.TOL_STATE[kb8]
    within(backend, "final chi2, relative" + tag, abs(stats[b, 1] - ost[1]) / ost[1], tc, (b,))
    within(backend, "initial chi2, relative" + tag, abs(stats[b, 4] - ost[4]) / ost[4], tc, (b,))
    within(backend, "final lambda, relative" + tag, abs(stats[b, 2] - ost[2]) / ost[2], tc, (b, stats[b, 2], ost[2]))
    for f in STATE_FIELDS:
        within(backend, "key-frame states" + tag, np.abs(kf[b, :nk][f] - o["kfs"][f]).max(), ts, (b, f))
    if nl:
        within(backend, "points" + tag, np.abs(pts[b, :nl] - o["points"]).max(), 10 * ts, (b,))
    still = (w["kfs"]["pose_fixed"] == 1) & ((w["kfs"]["has_imu"] == 0) | (w["kfs"]["imu_fixed"] == 1))
    assert np.array_equal(kf[b, :nk][still], w["kfs"][still]), "a fixed key frame moved"
    for f in ("pose_fixed", "has_imu", "imu_fixed"):
        assert np.array_equal(kf[b, :nk][f], w["kfs"][f])


def check_case(lib, backend, case, poison=True, errors=True):
    if CASES_ONLY:
        return None
    ws = case["windows"]
    stats, kf, pts, err = run_windows(lib, backend, ws, case["lam"], case["its"], poison, errors=errors)
    for b, (w, o) in enumerate(zip(ws, case["oracle"])):
        if errors:
            check_errors(backend, b, w, o["errors"], err)
        check_window(backend, b, w, o, stats, kf, pts)
    return stats, kf, pts, err


def batch_of(*cases):
    """several one-call cases with the same lambda and iteration count as one batch"""
    assert len({(c["lam"], c["its"]) for c in cases}) == 1
    return {"windows": sum((c["windows"] for c in cases), []), "oracle": sum((c["oracle"] for c in cases), []), "lam": cases[0]["lam"], "its": cases[0]["its"]}


# the first seeds from 100 on that satisfy, in the oracle alone, the premise, the margins and the conditioning check of inertial_cases.py
REJECTED = {"mono": (111, 3), "stereo": (108, 3), "fisheye": (100, 3)}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", ["mono", "stereo", "fisheye"])
def test_rejected_trials_restore_every_vertex(lib, backend, kind):
    """Free poses thrown 0.8 rad / 5 m off and lambda_init 1e-9: 11 to 12 trials in 3 iterations, most rejected.  After a rejected trial the pop must
    give back Rwb, twb, Rcw, tcw, v, bg, ba of every key frame with a free pose OR free IMU states, and the points: a state that is not restored
    changes currentChi's successor, the trial count and the final states."""
    case = K.cached(K.case_rejected, kind, *REJECTED[kind])
    assert "rejected trial" in K.reaches(case)
    check_case(lib, backend, case)


@pytest.mark.parametrize("backend", BACKENDS)
def test_rejected_trials_restore_a_fixed_pose_with_free_imu_states(lib, backend):
    """as above, with one key frame whose pose is fixed and whose velocity and biases are free (hp < 0, hi >= 0): a pop that goes by `hp` alone
    leaves its v, bg, ba at the rejected trial's values.  Seed: the only one in 100..159 that passes premise, margins and conditioning."""
    case = K.cached(K.case_rejected_fixed_pose_free_imu, 124, 3)
    assert "rejected trial" in K.reaches(case)
    check_case(lib, backend, case)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", ["stereo", "fisheye"])
def test_failed_factorisation_raises_lambda(lib, backend, kind):
    """a negative definite inertial information matrix: ok2 == false trials (tempChi = DBL_MAX, scale = 1e-3, pop) until lambda is large enough"""
    case = K.cached(K.case_cholesky, kind, 0)
    assert "ok2 == 0" in K.reaches(case)
    check_case(lib, backend, case)


@pytest.mark.parametrize("backend", BACKENDS)
def test_early_stops(lib, backend):
    """one run ended by nBad >= 3 after 3 of 8 iterations (stats[0] < iterations), one by the iterations cap"""
    nbad, cap = K.cached(K.case_stop_nbad, 0, 3e10), K.cached(K.case_stop_cap, 0)
    assert "stop: nBad >= 3" in K.reaches(nbad) and nbad["oracle"][0]["stats"][0] == 3 < nbad["its"]
    assert K.reaches(cap) == {"stop: iterations cap"}
    r = check_case(lib, backend, nbad)
    assert CASES_ONLY or r[0][0, 0] == 3
    check_case(lib, backend, cap)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("which", ["kb8", "kb8 camera-major", "kb8 duplicated", "pinhole duplicated"])
def test_obstab_codes(lib, backend, which):
    """code 2 (two adjacent edges of one pose: both cameras of the rig), code 3 (the pose's two edges apart after a camera-major sort; three edges of
    one pose, or two apart, after duplicating an edge at the end of the landmark's run).  Landmark-major order is all the ABI asks for."""
    case = K.cached(K.case_obstab, which, 5)
    assert ("obsTab code 3" in K.reaches(case)) == (which != "kb8")
    check_case(lib, backend, case)


VERTEX = ["no imu", "free pose, fixed imu", "fixed pose, free imu", "inactive inertial edge", "no visual edges", "free pose without visual edges",
          "landmarks without edges", "landmarks of fixed key frames only"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_vertex_configurations(lib, backend):
    """every index set-up the generator never produces, one window each, in one batch (the window without visual edges needs a neighbour: the
    wrapper asks for cap_e > 0)"""
    cases = [K.cached(K.case_vertex, v, 6) for v in VERTEX]
    r = check_case(lib, backend, batch_of(*cases))
    # the inertial edge between two fixed IMU key frames: reported by imu_chi2, absent from the robust sum
    w, o = cases[3]["windows"][0], cases[3]["oracle"][0]["errors"]
    active = dict(w, imu=w["imu"][:-1])
    assert o["imu_chi2"][-1, 0] > 1e-3 * o["robust_chi2_sum"] and O.inertial_errors(active, K.HUBER)["robust_chi2_sum"] == pytest.approx(o["robust_chi2_sum"], rel=1e-12)
    if r is not None:
        assert abs(r[3]["imu_chi2"][3, len(w["imu"]) - 1, 0] - o["imu_chi2"][-1, 0]) <= 1e-9 * max(1.0, o["imu_chi2"].max())


@pytest.mark.parametrize("backend", BACKENDS)
def test_counts_at_wave_lane_and_chunk_sizes(lib, backend):
    """1, 4, 5 free key frames (poses are dealt to four waves); a free pose with exactly 64 and with 70 visual edges (lanes stride by 64);
    255, 256, 257 visual edges (the counting sort's chunks of ceil(n / 256))"""
    check_case(lib, backend, batch_of(*[K.cached(K.case_free_count, n, 7) for n in (1, 4, 5)]))
    check_case(lib, backend, batch_of(*[K.cached(K.case_pose_edges, n, 8) for n in (64, 70)] + [K.cached(K.case_edge_count, n, 9) for n in (255, 256, 257)]))


@pytest.mark.gpu
def test_hip_32_free_key_frames(hip_lib):
    """nfp == LIBA_MAX_FREE: 32 free key frames, 480 reduced unknowns, 64 landmarks, 2 iterations"""
    check_case(hip_lib, "hip", K.cached(K.case_max_free, 10), errors=False)


@pytest.mark.parametrize("backend", BACKENDS)
def test_inertial_huber_above_and_below(lib, backend):
    """the Huber-carrying oldest inertial edge, active, with chi2 above 2 * 16.92 (rho1 < 1) and below 16.92 / 2"""
    check_case(lib, backend, batch_of(K.cached(K.case_inertial_huber, True, 11), K.cached(K.case_inertial_huber, False, 11)))


@pytest.mark.parametrize("backend", BACKENDS)
def test_ragged_batch_equals_windows_alone(lib, backend):
    """three windows of different n_kf / n_points / n_edges / n_imu in one call, poison in every slab's slack: each equals the oracle and, bit for
    bit, the same window run alone"""
    case = K.cached(K.case_ragged, 12)
    r = check_case(lib, backend, case)
    if r is None:
        return
    for b, w in enumerate(case["windows"]):
        st, kf, pts, err = run_windows(lib, backend, [w], case["lam"], case["its"], poison=False)
        assert np.array_equal(st[0], r[0][b]), (b, st[0], r[0][b])
        assert np.array_equal(kf[0].view(np.uint8), r[1][b, :len(w["kfs"])].view(np.uint8)) and np.array_equal(pts[0], r[2][b, :len(w["points"])])
        assert err["robust_chi2_sum"][0] == r[3]["robust_chi2_sum"][b]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("which", K.REFUSALS)
def test_refused_windows_are_left_untouched(lib, backend, which):
    """a valid and an invalid window in one liba_optimize call (liba_compute_errors does not validate and is not called): the invalid one reports
    stats = [-1, 0, 0, 0, 0] and keeps its key frames and points bit for bit; its neighbour is optimised as if alone"""
    good, bad, max_free = K.cached(K.case_refusal, which, 13)
    if CASES_ONLY:
        return
    ws = good["windows"] + [bad]
    stats, kf, pts, _ = run_windows(lib, backend, ws, good["lam"], good["its"], poison=True, max_free=max_free, errors=False)
    if max_free is None:
        check_window(backend, 0, ws[0], good["oracle"][0], stats, kf, pts)
    else:       # the valid neighbour has as many free poses as the lowered max_free allows
        assert len(K.free_poses(ws[0])) == max_free
        check_window(backend, 0, ws[0], good["oracle"][0], stats, kf, pts)
    assert stats[1].tolist() == [-1, 0, 0, 0, 0], stats[1]
    assert np.array_equal(kf[1, :len(bad["kfs"])].view(np.uint8), bad["kfs"].view(np.uint8)), "a refused window's key frames changed"
    assert np.array_equal(pts[1, :len(bad["points"])], bad["points"]), "a refused window's points changed"


# measured on the CPU, dense_lm_step against the oracle, largest of key-frame states and points: 2.8e-14 (stereo), 7.0e-14 (KB8).
# Ten times the larger figure, since the Schur elimination reorders the sums.
DENSE_TOL = 7e-13


@pytest.mark.parametrize("kind", ["stereo", "fisheye"])
def test_dense_normal_equations_match_the_oracle(kind):
    """One LM step without the Schur complement: the full normal equations over [poses | V, G, A | points] from the oracle's per-edge errors and
    Jacobians, solved by numpy.linalg.solve, against the oracle's optimize(lambda, 1).  What the two share is the edge linearisation (pinned by central
    differences in test_inertial_parity.py); the elimination, the back-substitution and the index set-up are independent."""
    case = K.cached(K.case_dense, kind, 14)
    dkf, dpts = case["dense"]
    o = case["oracle"][0]
    dev = max(max(np.abs(dkf[f] - o["kfs"][f]).max() for f in STATE_FIELDS), np.abs(dpts - o["points"]).max())
    print("dense step vs oracle (%s): %.3e" % (kind, dev))
    assert dev <= DENSE_TOL, dev


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", ["stereo", "fisheye"])
def test_dense_normal_equations_match_the_kernel(lib, backend, kind):
    """The same dense step against the kernel's state after optimize(lambda, 1).  Pinhole: DENSE_TOL, as for the oracle (seen: 1.5e-14 on the emulator
    and on the MI355X).  KB8: the dense step is built from the oracle's projections, and the kernel's atan2f differs from the oracle's float(atan2)
    (DESIGN.md section 2), which no reordering of sums explains; the bar there is this file's KB8 state bar (seen: 4.6e-8 on states, 1.2e-6 on points)."""
    case = K.cached(K.case_dense, kind, 14)
    if CASES_ONLY:
        return
    w = case["windows"][0]
    stats, kf, pts, _ = run_windows(lib, backend, [w], case["lam"], 1, poison=False, errors=False)
    assert stats[0, 0] == 1 and stats[0, 3] == 1
    dkf, dpts = case["dense"]
    kb8 = kind == "fisheye"
    for f in STATE_FIELDS:
        within(backend, "dense step, key-frame states (%s)" % kind, np.abs(kf[0][f] - dkf[f]).max(), K.TOL_STATE[kb8] if kb8 else DENSE_TOL, (f,))
    within(backend, "dense step, points (%s)" % kind, np.abs(pts[0] - dpts).max(), 10 * K.TOL_STATE[kb8] if kb8 else DENSE_TOL)


# ---- liba_pose_inertial_kf / liba_pose_inertial_lastframe -------------------------------------------------------------------------------------
def check_pose_case(lib, backend, case):
    if CASES_ONLY:
        return
    fs, lastframe, rec = case["frames"], case["lastframe"], case["rec_init"]
    B, cap = len(fs), max(len(f["edges"]) for f in fs) + 7
    edges, n = np.zeros((B, cap), POSE_EDGE_DTYPE), np.array([len(f["edges"]) for f in fs], np.int32)
    for b, f in enumerate(fs):
        edges[b, :n[b]] = f["edges"]
    K.poison_pose_edges(edges, n)
    cat = lambda k: np.concatenate([f[k] for f in fs])      # noqa: E731
    up = lambda a: to_dev_plain(a, backend)                 # noqa: E731
    rigs = [f["rig"] for f in fs]
    if lastframe:
        fr, pv, outl, H, good = pose_inertial_optimization_last_frame(cat("frame"), cat("keyframe"), rigs, edges, n, cat("imu"), cat("prior"), up, rec_init=rec, lib=lib)
    else:
        fr, outl, H, good = pose_inertial_optimization_last_keyframe(cat("frame"), cat("keyframe"), rigs, edges, n, cat("imu"), up, rec_init=rec, lib=lib)
    name = "lastframe" if lastframe else "kf"
    for b, (f, o) in enumerate(zip(fs, case["oracle"])):
        kb8 = f["rig"].model[0] == 1
        tag = " (KB8)" if kb8 else " (pinhole)"
        assert good[b] == o["n_good"], (b, good[b], o["n_good"])
        assert np.array_equal(outl[b, :n[b]], o["outlier"]), (b, np.flatnonzero(outl[b, :n[b]] != o["outlier"]))
        assert (outl[b, n[b]:] == 0).all(), "an outlier flag was written in the slack"
        for fld in STATE_FIELDS:
            within(backend, "pose_inertial_%s frame states%s" % (name, tag), np.abs(fr[b][fld] - o["frame"][0][fld]).max(), K.TOL_STATE[kb8], (b, fld))
            if lastframe:
                within(backend, "pose_inertial_lastframe previous frame%s" % tag, np.abs(pv[b][fld] - o["prev"][0][fld]).max(), K.TOL_STATE[kb8], (b, fld))
        assert np.isfinite(o["H"]).all() and np.isfinite(H[b]).all(), b
        bar = 1e-3 if kb8 else (1e-5 if lastframe else 1e-6)      # the bars of test_inertial_parity.py
        within(backend, "pose_inertial_%s H / max%s" % (name, tag), np.abs(H[b] - o["H"]).max() / np.abs(o["H"]).max(), bar, (b,))


COUNT_SEEDS = (200, 200, 200, 200, 201, 200, 200, 200)          # first seeds from 200 whose classifications all have margin
RECOVERY_SEEDS = {False: (301, 300, 300, 301), True: (301, 300, 300, 300)}      # first seeds from 300 with a truncation at 29 / 30 inliers and margin
SPECIAL_SEEDS = {False: (400, 410, 420, 505), True: (400, 410, 420, 500)}       # [3]: first seed from 500 with an edge out in one round, in again later


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("lastframe", [False, True], ids=["kf", "lastframe"])
def test_pose_inertial_edge_counts(lib, backend, lastframe):
    """n_edges 0, 5, 6, 7, 63, 64, 65, 129 in one batch: 5, 6, 7 straddle `edges().size() < 10` (ne + 3 for LastKeyFrame, ne + 4 for LastFrame:
    one round instead of four), 63 / 64 / 65 / 129 the lane-stride loops"""
    check_pose_case(lib, backend, K.cached(K.case_edge_counts, lastframe, COUNT_SEEDS))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("rec_init", [False, True], ids=["rec0", "rec1"])
@pytest.mark.parametrize("lastframe", [False, True], ids=["kf", "lastframe"])
def test_pose_inertial_recovery_at_29_and_30_inliers(lib, backend, lastframe, rec_init):
    """frames truncated to 29 and to 30 inliers after round 4: the recovery pass runs only for 29 with rec_init = 0, and re-admits edges"""
    case = K.cached(K.case_recovery, lastframe, rec_init, RECOVERY_SEEDS[lastframe])
    assert [r["trace"]["recovery"] for r in case["oracle"]] == [not rec_init, False, not rec_init, False]
    check_pose_case(lib, backend, case)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("lastframe", [False, True], ids=["kf", "lastframe"])
def test_pose_inertial_special_edges(lib, backend, lastframe):
    """points behind the camera with a small chi2 (only !depthPositive rejects them); mono edges with and without bClose between chi2Mono and
    1.5 * chi2Mono; a frame whose reprojection edges are all out after round 1 (inertial-only system, n_good 0); an edge out in one round and in
    again in a later one (`if (outl[e]) chiLast[e] = chi2` at the current state)"""
    check_pose_case(lib, backend, K.cached(K.case_special_edges, lastframe, SPECIAL_SEEDS[lastframe]))


@pytest.mark.parametrize("backend", BACKENDS)
def test_lastframe_prior_huber(lib, backend):
    """EdgePriorPoseImu with chi2 above 25 at every step (1500 ... 3750: Huber weight below 1) and below (0.2 ... 1.3)"""
    check_pose_case(lib, backend, K.cached(K.case_prior, 50))


@pytest.mark.parametrize("backend", BACKENDS)
def test_lastframe_marginalisation_drops_zero_singular_values(lib, backend):
    """H_pp with three singular values of exactly 0 (no gyro-bias information at all) and every other one above 2.5e3: the pseudo-inverse must skip
    them (`sv > 1e-6`), or the prior handed on is not finite.  Gauss-Newton's factorisation fails at the first step, so the states stay put."""
    case = K.cached(K.case_dropped_sv, 60)
    tr = case["oracle"][0]["trace"]
    assert tr["sv_dropped"] == 3 and tr["sv_kept"] == 12 and (tr["gn_steps"] == 0).all()
    check_pose_case(lib, backend, case)
