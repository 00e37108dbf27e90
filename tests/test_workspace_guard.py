"""Nothing is written behind a workspace: every entry point that takes a caller-allocated workspace runs once on a buffer of
*_workspace_bytes + 4096 whose tail holds a byte pattern, and the tail is intact afterwards.

No entry point receives its buffer's size, so a layout function that sizes a section differently from how a kernel
indexes it writes past the allocation, silently on the CPU tier and as a fault on the GPU.  The shapes are the smallest that reach every
section: odd counts, and for lba_optimize one window per launch plan (the plan is asserted first, as in test_lm_solver_plans.py).  The buffer
goes in through the wrappers: `work=` where they take one, else their cached workspace attribute.

What this does not prove: the buffer's size comes from the layout function under test, so only a write behind the LAST byte of the whole
layout is seen.  A section inside the layout that is sized too small overlaps its neighbour without touching the tail; that shows, if at
all, in the results the other tests compare."""
import ctypes as C

import numpy as np
import pytest

import orbhip
from devarrays import BACKENDS, lib, to_dev, to_dev_plain, to_host, uploader  # noqa: F401  (lib: the fixture of the tests parametrised over BACKENDS)
from orbhip import _lib
from orbhip.inertial import InertialWindows, synth_inertial_window
from orbhip.lba import LbaWindows, synth_window
from orbhip.matcher import LOCALMAP_FRAME_DTYPE, MODE_BEST_ONLY, MODE_LOCAL_MAP, Q_RIGHT, Q_TWIN, QUERY_DTYPE

CANARY, TAIL = 0xA7, 4096


def guarded(nbytes, backend, dtype=np.uint8):
    """a zeroed workspace of nbytes with TAIL canary bytes behind it, as an array of `dtype` on the backend"""
    a = np.zeros(nbytes + TAIL, np.uint8)
    a[nbytes:] = CANARY
    return to_dev_plain(a.view(dtype), backend)


def assert_tail_intact(buf, nbytes, backend):
    if backend == "hip":
        import torch
        torch.cuda.synchronize()
    tail = to_host(buf).view(np.uint8).reshape(-1)[nbytes:]
    assert len(tail) == TAIL and (tail == CANARY).all(), ("written behind the workspace at byte", nbytes + int(np.nonzero(tail != CANARY)[0][0]))


# ---- SearchByProjection -------------------------------------------------------------------------------------------------------------------------
def sbp_slabs(backend, frames, cap_k, cap_q):
    """test_resolver_rounds.run_frames' slabs with the capacities given"""
    B = len(frames)
    kps = np.zeros((B, cap_k, 7), np.float32); desc = np.zeros((B, cap_k, 32), np.uint8)
    Q = np.zeros((B, cap_q), QUERY_DTYPE); qd = np.zeros((B, cap_q, 32), np.uint8)
    nk = np.zeros(B, np.int32); nq = np.zeros(B, np.int32)
    for b, (k, d, q, qdd) in enumerate(frames):
        kps[b, :len(k)] = k.view(np.float32).reshape(-1, 7); desc[b, :len(k)] = d; nk[b] = len(k)
        Q[b, :len(q)] = q; qd[b, :len(q)] = qdd; nq[b] = len(q)
    dv = lambda a: to_dev_plain(a, backend)   # noqa: E731
    return dv(kps), dv(desc), dv(nk), dv(Q.view(np.uint8).reshape(B, cap_q, 28)), dv(qd), dv(nq)


def sbp_frames():
    from test_resolver_rounds import crowded_frame
    rng = np.random.default_rng(11)
    return [crowded_frame(rng, 2, 4, n) for n in (5, 4, 3)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", [MODE_BEST_ONLY, MODE_LOCAL_MAP])
def test_search_by_projection_fused(lib, backend, mode):
    """3 frames, cap_q 5, on k_sbp_frame; frame 1 carries a rig twin, which k_sbp_frame hands to the one-wave walk: its flag word (the
    workspace's last section) is written, and its query rows are rewritten by the fallback kernels"""
    from test_resolver_rounds import GRID
    frames = sbp_frames()
    frames[1][2]["flags"][1] |= Q_TWIN
    B, cap_k, cap_q = 3, 11, 5
    kps, desc, nk, Q, qd, nq = sbp_slabs(backend, frames, cap_k, cap_q)
    m = orbhip.ORBmatcher(0.9, True, lib=lib)
    gs, gi = m.grid_build(kps, nk, GRID)
    nbytes = lib.orbm_search_workspace_bytes(B, cap_q)
    work = guarded(nbytes, backend)
    _, _, nm = m.SearchByProjection(kps, desc, nk, gs, gi, Q, qd, nq, GRID, mode, 255, work=work)
    assert_tail_intact(work, nbytes, backend)
    flags = to_host(work)[nbytes - 16:nbytes].view(np.int32)[:B]   # one flag word per frame, padded to 16 bytes, ends the workspace
    assert flags.tolist() == [0, 1, 0], flags
    assert to_host(nm).sum() > 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_search_by_projection_rig(lib, backend, monkeypatch):
    """the rig entry point (k_sbp_candidates2 -> k_sbp_resolve on every frame).  SearchByProjectionRig allocates its workspace itself: the
    allocation of exactly that size is answered with the guarded buffer"""
    from test_resolver_rounds import GRID
    import orbhip.matcher as M
    frames = sbp_frames()
    for f in frames:
        f[2]["flags"][1::2] |= Q_RIGHT | Q_TWIN
    B, cap_k, cap_q = 3, 11, 5
    kps, desc, nk, Q, qd, nq = sbp_slabs(backend, frames, cap_k, cap_q)
    m = orbhip.ORBmatcher(0.9, True, lib=lib)
    gs, gi = m.grid_build_rig(kps, nk, to_dev_plain(np.full(B, 4, np.int32), backend), GRID)
    nbytes = lib.orbm_search_workspace_bytes(B, cap_q)
    work, handed = guarded(nbytes, backend), []

    def zeros(like, shape, dtype):
        if tuple(shape) == (nbytes,) and dtype == np.uint8:
            handed.append(work)
            return work
        return _lib.zeros(like, shape, dtype)
    monkeypatch.setattr(M, "zeros", zeros)
    m.SearchByProjectionRig(kps, desc, nk, gs, gi, Q, qd, nq, GRID, MODE_BEST_ONLY, 255)
    assert len(handed) == 1
    assert_tail_intact(work, nbytes, backend)


# ---- Sim3Solver ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_sim3_solve(lib, backend):
    """batch 2, cap_its 3: every hypothesis row of the workspace is written (no problem converges early: all its iterations are evaluated)"""
    from orbhip.sim3 import Sim3Solver
    from test_sim3_solver import device, scene
    probs = [scene(70, 24, 23, 3, outliers=0.5), scene(71, 17, 16, 3, outliers=0.5, fix_scale=1)]
    S = Sim3Solver(2, 24, 3, max(int(P["n1"]) for P, *_ in probs), device=device(backend), lib=lib)
    nbytes = lib.orbm_sim3_workspace_bytes(2, 24, 3)
    assert nbytes == to_host(S._work).nbytes
    S._work = guarded(nbytes, backend, np.int64)
    S.solve(np.array([P for P, *_ in probs]), [C for _, C, *_ in probs], [s for _, _, s, *_ in probs])
    assert_tail_intact(S._work, nbytes, backend)
    assert (S.to_host()["result"]["iterations"] == 3).all()


# ---- UpdateLocalMap -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_update_local_map(lib, backend):
    """2 frames on 5 key frames and 7 points: the slice of a frame is 47 words, padded to 48"""
    from test_local_map import _rows, frame_points, random_world
    rng = np.random.default_rng(21)
    W = random_world(rng, 5, 7, 4, B=2, p_bad_kf=0.0, p_bad_mp=0.0)
    votes = [frame_points(rng, W, 6), frame_points(rng, W, 5)]
    vote_a, n_vote = _rows(votes, 9, 2)
    fr = np.zeros(2, LOCALMAP_FRAME_DTYPE)
    fr["last_kf"] = -1
    m = orbhip.ORBmatcher(0.8, True, lib=lib)
    nbytes = lib.orbm_local_map_workspace_bytes(5, 7, 2)
    assert nbytes == 2 * 48 * 4
    work = guarded(nbytes, backend, np.int32)
    d_vote, d_n = to_dev_plain(vote_a, backend), to_dev_plain(n_vote, backend)
    out = m.UpdateLocalMap(W.view(backend), to_dev(fr, backend), d_vote, d_n, d_vote, d_n, 8, 7, work=work)
    assert_tail_intact(work, nbytes, backend)
    m.check_local_map(out)
    assert to_host(out["nmp"]).sum() > 0 and to_host(out["n_local_kf"]).sum() > 0


# ---- KeyFrameDatabase ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("family", ["reloc", "place"])
def test_keyframe_database_queries(lib, backend, family):
    """5 slots and 3 queries (odd counts: every section is padded), compared with the restatement as in test_keyframe_database.py"""
    from test_keyframe_database import simple_bow, small_pair
    bows = [simple_bow([3, 5, 9, 12]), simple_bow([1, 5, 9, 12, 20]), simple_bow([0, 3, 5, 9, 12]), simple_bow([2, 3, 9]), simple_bow([5, 9, 12, 30])]
    P = small_pair(lib, backend, bows, maps=[0, 0, 1, 0, 1], covis=[[1, 2], [0], [0, 3], [2], []])
    nbytes = lib.bowdb_workspace_bytes(5, 3)
    work = P.db._work[3] = guarded(nbytes, backend, np.int64)
    qs = [simple_bow([3, 5, 9, 12]), simple_bow([5, 9, 12, 20]), simple_bow([40, 41])]
    if family == "reloc":
        want, _, _ = P.reloc([4, 5, 9], qs, [0, 1, 0])
    else:
        want, _, _ = P.nbest([4, 5, 9], qs, [0, 1, 0], [[1], [], [0, 4]])
    assert P.db._work[3] is work and any(len(w) for w in want)
    assert_tail_intact(work, nbytes, backend)


# ---- liba_optimize ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_liba_optimize(lib, backend):
    """2 small inertial windows of different sizes: the second one's slice ends the workspace"""
    ws = [synth_inertial_window(30 + i, n_opt=2 + i, n_fixed_vis=1, n_pts=20 + 7 * i, max_obs=3, kind=k) for i, k in enumerate(("stereo", "mono"))]
    IW = InertialWindows(ws, uploader(backend), lib=lib)
    nbytes = lib.liba_workspace_bytes(C.byref(IW.prob), IW.B)
    IW._work = work = guarded(nbytes, backend)
    stats = to_host(IW.optimize(1.0, 2))
    assert IW._work is work
    assert_tail_intact(work, nbytes, backend)
    assert (stats[:, 0] >= 1).all(), stats


# ---- lba_optimize: one window (or batch) per launch plan ------------------------------------------------------------------------------------------
def small_window(seed, nfree, npts):
    return synth_window(seed, nfree + 1, 1, npts, min(8, nfree + 1), "stereo")


def lba_case(plan, backend, default_lib):
    """-> (library, windows, cameras, the entries of lm_plan's dict the case is written for).  The split rows and the global-memory panel need 1100
    edges on 2 free poses and 177 free key frames with the default constants (GPU tier); the CPU tier reaches them in the forced-path emulator
    builds of test_lba_parity.py"""
    if plan == "per_panel":                 # batch 1, 6 free key frames: cholL / cholY / cholX
        w, cams = small_window(50, 6, 60)
        return default_lib, [w], cams, dict(chol=0, schur_g=1, pan_global=0)
    if plan == "one_workgroup":             # 49 windows: no per-panel sections, the LDS panel
        # the smallest windows there are, 1 free pose and 8 points: the plan needs the batch of 49, and the emulator runs every one of its
        # workgroups fiber by fiber (512 fibers per factorisation), which is what this case's time goes to on the CPU tier
        built = [small_window(60 + i % 2, 1, 8) for i in range(49)]
        return default_lib, [b[0] for b in built], built[0][1], dict(chol=2, schur_g=1, pan_global=0, step_ws=0)
    variant = None
    if plan == "split_rows":                # schurPart
        w, cams = small_window(51, 2, 900 if backend == "hip" else 40)
        assert backend == "emu" or len(w["edges"]) >= 1100
        variant, want = (("LM_SCHUR_SPLIT_MIN_EDGES=4",), "schursplit"), dict(split_ws=1)
    else:                                   # panExt
        w, cams = small_window(52, 177, 300) if backend == "hip" else small_window(52, 6, 60)
        variant, want = (("WG_CHOL_LDS_MAX_LD=30", "LM_CHOL_SPLIT_MAX_BATCH=0"), "cholext"), dict(chol=3, pan_global=1)
    if backend == "emu":
        import build_emu
        return _lib.bind(C.CDLL(build_emu.build(defines=variant[0], tag=variant[1]))), [w], cams, want
    return default_lib, [w], cams, want


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("plan", ["per_panel", "one_workgroup", "split_rows", "global_panel"])
def test_lba_optimize(lib, backend, plan):
    from test_lm_solver_plans import lm_plan
    L_, ws, cams, want = lba_case(plan, backend, lib)
    L = LbaWindows(ws, cams, uploader(backend), lib=L_)
    got = lm_plan(L_, L.B, L.cap_p, L.cap_l, L.cap_e, max(int((w["pose_hidx"] >= 0).sum()) for w in ws))
    for k, v in want.items():
        assert got[k] == v, "this case no longer takes the plan it was written for: %s = %s, not %s (%s)" % (k, got[k], v, got)
    assert got["split_ws"] == (got["schur_g"] > 1)
    P, _ = L._structs(())
    nbytes = L_.lba_lm_workspace_bytes(C.byref(P), L.B)
    L._lm_ws = work = guarded(nbytes, backend)
    stats = L.optimize(1)   # one iteration = the linearisation and at least one lambda trial: every kernel of the loop has run
    assert L._lm_ws is work
    assert_tail_intact(work, nbytes, backend)
    assert (stats[:, 0] >= 1).all() and np.isfinite(stats).all(), stats
