"""The mapping-side matcher kernels (k_bow, k_tri, k_fuse, k_mutual, the ORBM_MODE_INIT resolver, k_hamming, k_knn2) on the constructed cases
of tests/matcher_cases.py: ties, thresholds, node and window sizes across the 64-entry chunks, ragged batches with traps in the slack.

Every case is checked three ways, all by exact equality of indices, distances and counts: kernel against the oracle, oracle against the
outcome planted in the builder, kernel against the planted outcome.  The planted outcomes follow the text of the reference's
src/ORBmatcher.cc.  One of them differs from what one would write down without float arithmetic: at mfNNratio = 0.6 the pair
(bestDist1, bestDist2) = (30, 50) PASSES `(float)30 < 0.6f * (float)50`, because 0.6f * 50.0f rounds up to 30.000002f; (31, 50) is the first
to fail.  The exact boundary is taken at ratio 0.5 (25 < 25.0f fails)."""
import numpy as np
import pytest

import matcher_cases as M
import oracle_lib as O
import orbhip
from devarrays import BACKENDS, lib, to_dev_plain, to_host  # noqa: F401
from orbhip._lib import check, ptr, stream, zeros
from orbhip.matcher import TH_LOW

_CACHE = {}


def cached(fn, *a):
    """a builder's result, built once per argument list and left unchanged"""
    key = (fn.__name__,) + a
    if key not in _CACHE:
        _CACHE[key] = fn(*a)
    return _CACHE[key]


def same(a, b, what):
    assert np.array_equal(np.asarray(a), np.asarray(b)), "%s\n got  %s\n want %s" % (what, np.asarray(a).tolist(), np.asarray(b).tolist())


def three_way(kernel, oracle, planted, what):
    same(oracle, planted, what + ": oracle against the planted outcome")
    same(kernel, planted, what + ": kernel against the planted outcome")
    same(kernel, oracle, what + ": kernel against the oracle")


# ---- SearchByBoW --------------------------------------------------------------------------------------------------------------------
def _bow_dev(s, backend, rig=False):
    keys = ("desc", "angle", "node_id", "node_start", "feat_idx", "n_nodes") + (("n_left",) if rig else ())
    return {k: to_dev_plain(s[k], backend) for k in keys}


def _bow_check(lib, backend, cases, kk, ratio, ori, rig=False):
    """cases: per batch entry (outer, inner, {outer label: inner label} or [(outer, inner)], empty)"""
    outers = [M.as_empty(c[0]) if c[3] else c[0] for c in cases]
    inners = [M.as_empty(c[1]) if c[3] else c[1] for c in cases]
    so = M.pack_sides(outers, inners, max(o["n"] for o in outers), max(o["n_nodes"] for o in outers), trap_node_of=lambda b: M.BACK_NODE)
    si = M.pack_sides(inners, outers, max(i["n"] for i in inners), max(i["n_nodes"] for i in inners))
    assert min(o["n"] for o in outers) < so["desc"].shape[1] and min(i["n"] for i in inners) < si["desc"].shape[1]   # there IS slack
    m = orbhip.ORBmatcher(ratio, ori, lib=lib)
    d = lambda a: to_dev_plain(a, backend)   # noqa: E731
    if kk:
        got, cnt = [to_host(x) for x in m.SearchByBoWKF(_bow_dev(so, backend), d(so["valid"]), _bow_dev(si, backend), d(si["valid"]))]
    else:
        got, cnt = [to_host(x) for x in m.SearchByBoW(_bow_dev(so, backend), d(so["valid"]), _bow_dev(si, backend, rig))]
    for b, (o, i, exp, empty) in enumerate(cases):
        pairs = exp if isinstance(exp, dict) else None
        if empty:
            want, n = np.full(o["n"] if kk else i["n"], -1, np.int32), 0
        elif pairs is not None:
            want, n = M.expect_array(pairs, o, i, by_dst=not kk)
        else:       # a list of pairs: one outer feature may hold a left and a right match (rig)
            want, n = np.full(i["n"], -1, np.int32), len(exp)
            for a, c in exp:
                want[i["index"][c]] = o["index"][a]
        oo, oi = dict(M.oracle_side(o), n_nodes=0 if empty else o["n_nodes"]), dict(M.oracle_side(i), n_nodes=0 if empty else i["n_nodes"])
        if kk:
            om, on = O.search_by_bow_kf(oo, o["valid"], oi, i["valid"], ratio, ori)
        else:
            om, on = O.search_by_bow(oo, o["valid"], oi, ratio, ori, i["n_left"] if rig else -1)
        nout = len(want)
        three_way(got[b, :nout], om, want, "entry %d matches" % b)
        three_way(cnt[b], on, n, "entry %d count" % b)
        assert (got[b, nout:] == -1).all(), "entry %d: a slack feature was matched" % b


def _batch(build, args0, args1, args2):
    """B = 3: a partly filled entry, one that fills the slabs (pad > 0) and an empty one (all its data in place, counts 0)"""
    return [cached(build, *args0) + (False,), cached(build, *args1) + (False,), cached(build, *args2) + (True,)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kk", [False, True], ids=["kf_f", "kf_kf"])
def test_bow_nodes_thresholds_ties(lib, backend, kk):
    """Inner node sizes 1, 2, 63, 64, 65, 130 with the best at 0, 1, 0, 63, 64, 129; best distance 49 / 50 / 51 (`<= TH_LOW` :464 against
    `< TH_LOW` :1067); equal and near-equal bests in different chunks; an inner feature taken by an earlier outer one; invalid features on
    both sides; nodes on one side only at the front, middle and back."""
    _bow_check(lib, backend, _batch(M.bow_main_case, (11, kk, 0), (12, kk, 9), (13, kk, 2)), kk, M.BOW_RATIO, True)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kk", [False, True], ids=["kf_f", "kf_kf"])
@pytest.mark.parametrize("ratio", [0.6, 0.5])
def test_bow_ratio_boundary(lib, backend, kk, ratio):
    big = cached(M.bow_rotation_case, 24)       # the entry that fills the slabs: 13 lone candidates at distance 10 pass any ratio
    cases = [cached(M.bow_ratio_case, 21, ratio, kk) + (False,), (big[0], big[1], big[3], False), cached(M.bow_ratio_case, 23, ratio, kk) + (True,),
             cached(M.bow_ratio_case, 22, ratio, kk) + (False,)]
    _bow_check(lib, backend, cases, kk, ratio, False)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n_left", ["split", "all", "none"])
def test_bow_rig(lib, backend, n_left):
    """F.Nleft in {N / 2, N, 0}: the right camera's match rides on the left best passing TH_LOW and skips the ratio test"""
    big = cached(M.bow_main_case, 12, False, 9)
    cases = [cached(M.bow_rig_case, 31, n_left) + (False,), cached(M.bow_rig_case, 32, n_left) + (False,),
             cached(M.bow_rig_case, 33, n_left) + (True,), (big[0], dict(big[1], n_left=0), [], False)]   # the last fills the slabs: Nleft = 0, no match
    _bow_check(lib, backend, cases, False, 0.9, True, rig=True)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kk", [False, True], ids=["kf_f", "kf_kf"])
@pytest.mark.parametrize("ori", [True, False])
def test_bow_rotation_histogram(lib, backend, kk, ori):
    """equal counts in several bins (the first ones in bin order stay) and a second maximum of exactly one tenth of the first (it stays)"""
    def case(seed):
        o, i, on, off = cached(M.bow_rotation_case, seed)
        return o, i, on if ori else off
    main = cached(M.bow_main_case, 12, kk, 9)
    _bow_check(lib, backend, [case(41) + (False,), case(42) + (False,), case(43) + (True,), main + (False,)], kk, 0.9, ori)


# ---- SearchForTriangulation ---------------------------------------------------------------------------------------------------------
def _tri_dev(s, backend):
    return {k: to_dev_plain(s[k], backend) for k in ("kps", "desc", "u_right", "has_mp", "node_id", "node_start", "feat_idx", "n_nodes")}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("only_stereo,coarse", [(False, False), (False, True), (True, False)], ids=["plain", "coarse", "only_stereo"])
def test_triangulation_pinhole(lib, backend, only_stereo, coarse):
    """KF2 node sizes; the LAST of equal distances (positions 3 and 70); a nearest candidate that fails the epipolar gate; a later equal
    one that fails it; two KF1 features on one KF2 feature; the epipole gate per octave; u_right of -1, 0.0 and positive; bOnlyStereo;
    map points on either side; distance 50 / 51; F12 = 0 (entry 3) with and without bCoarse."""
    mode = "only_stereo" if only_stereo else "coarse" if coarse else "plain"
    built = [cached(M.tri_case, 51, 0), cached(M.tri_case, 52, 6), cached(M.tri_case, 53, 1), cached(M.tri_case, 54, 3)]
    empty = [False, False, True, False]
    f0 = [False, False, False, True]
    k1 = [M.as_empty(c[0]) if e else c[0] for c, e in zip(built, empty)]
    k2 = [M.as_empty(c[1]) if e else c[1] for c, e in zip(built, empty)]
    s1 = M.pack_sides(k1, k2, max(s["n"] for s in k1), max(s["n_nodes"] for s in k1), trap_node_of=lambda b: M.BACK_NODE)
    s2 = M.pack_sides(k2, k1, max(s["n"] for s in k2), max(s["n_nodes"] for s in k2))
    pairs = M.tri_pairs(f0)
    m = orbhip.ORBmatcher(0.6, True, lib=lib)
    got, cnt = [to_host(x) for x in m.SearchForTriangulation(_tri_dev(s1, backend), _tri_dev(s2, backend),
                                                             to_dev_plain(pairs.view(np.uint8).reshape(len(built), -1), backend), only_stereo, coarse)]
    for b, (a, c, exp) in enumerate(built):
        key = ("f0_coarse" if coarse else "f0") if f0[b] else mode
        pl = {} if empty[b] or (f0[b] and only_stereo) else exp[key]
        want, n = M.expect_array(pl, a, c, by_dst=False)
        oa, oc = dict(M.oracle_side(a), n_nodes=0 if empty[b] else a["n_nodes"]), dict(M.oracle_side(c), n_nodes=0 if empty[b] else c["n_nodes"])
        om, on = O.search_for_triangulation(oa, oc, pairs["F12"][b], M.TRI_EP, M.TRI_SIGMA2, M.TRI_SCALE, only_stereo, coarse, True)
        three_way(got[b, :a["n"]], om, want, "entry %d vMatches12" % b)
        three_way(cnt[b], on, n, "entry %d count" % b)
        assert (got[b, a["n"]:] == -1).all(), "entry %d: a slack feature was matched" % b
    if mode == "plain":   # the duplicate is really there: two KF1 features hold one KF2 feature
        w = M.expect_array(built[0][2]["plain"], built[0][0], built[0][1], by_dst=False)[0]
        assert len(np.unique(w[w >= 0])) == (w >= 0).sum() - 1


@pytest.mark.parametrize("backend", BACKENDS)
def test_triangulation_kb8_coarse(lib, backend):
    """the same key frames through k_tri<KB8> with one fisheye camera each and bCoarse: node sizes, the last of equal distances, the
    epipole gate, map points, ragged entries; no feature is stereo"""
    built = [cached(M.tri_case, 51, 0), cached(M.tri_case, 52, 6), cached(M.tri_case, 53, 1)]
    empty = [False, False, True]
    k1 = [M.as_empty(c[0]) if e else c[0] for c, e in zip(built, empty)]
    k2 = [M.as_empty(c[1]) if e else c[1] for c, e in zip(built, empty)]
    s1 = M.pack_sides(k1, k2, max(s["n"] for s in k1), max(s["n_nodes"] for s in k1), trap_node_of=lambda b: M.BACK_NODE)
    s2 = M.pack_sides(k2, k1, max(s["n"] for s in k2), max(s["n_nodes"] for s in k2))
    pairs = M.tri_kb8_pairs(len(built))
    nl = to_dev_plain(np.full(len(built), -1, np.int32), backend)
    m = orbhip.ORBmatcher(0.6, True, lib=lib)
    got, cnt = [to_host(x) for x in m.SearchForTriangulationKB8(_tri_dev(s1, backend), _tri_dev(s2, backend), nl, nl,
                                                                to_dev_plain(pairs.view(np.uint8).reshape(len(built), -1), backend), False, True)]
    for b, (a, c, exp) in enumerate(built):
        want, n = M.expect_array({} if empty[b] else exp["kb8_coarse"], a, c, by_dst=False)
        oa, oc = dict(M.oracle_side(a), n_nodes=0 if empty[b] else a["n_nodes"]), dict(M.oracle_side(c), n_nodes=0 if empty[b] else c["n_nodes"])
        om, on = O.search_for_triangulation_kb8(oa, oc, -1, -1, pairs[b:b + 1], False, True, True)
        three_way(got[b, :a["n"]], om, want, "entry %d vMatches12" % b)
        three_way(cnt[b], on, n, "entry %d count" % b)
        assert (got[b, a["n"]:] == -1).all(), "entry %d: a slack feature was matched" % b


# ---- Fuse / SearchBySim3 / the agreement pass -----------------------------------------------------------------------------------------
def _query_bytes(q, backend):
    return to_dev_plain(q.view(np.uint8).reshape(q.shape + (28,)), backend)


def _fuse_check(lib, backend, entries, th, inv_sigma2):
    """entries: per batch entry (frame, queries, qdesc, expected, nq used)"""
    B = len(entries)
    cap_k = max(e[0]["n"] for e in entries)
    cap_q = max(len(e[1]) for e in entries) + 3
    assert cap_q % 4 and min(e[0]["n"] for e in entries) < cap_k
    # traps: behind n key points that sit on the first query with its descriptor, behind nq valid copies of the queries
    kps = M.pack_rows([e[0]["kps"] for e in entries], cap_k, [np.array([M.keypoint(e[1][0]["u"], e[1][0]["v"])], M.KP_DTYPE) for e in entries])
    desc = M.pack_rows([e[0]["desc"] for e in entries], cap_k, [e[2][:1] for e in entries])
    ur = M.pack_rows([e[0]["u_right"] for e in entries], cap_k, [np.full(1, -1, np.float32)] * B)
    nk = np.array([e[0]["n"] for e in entries], np.int32)
    nq = np.array([e[4] for e in entries], np.int32)
    qs = M.pack_rows([e[1][:e[4]] for e in entries], cap_q, [e[1] for e in entries])
    qd = M.pack_rows([e[2][:e[4]] for e in entries], cap_q, [e[2] for e in entries])
    m = orbhip.ORBmatcher(lib=lib)
    d = lambda a: to_dev_plain(a, backend)   # noqa: E731
    dk, dn = d(kps.view(np.float32).reshape(B, cap_k, 7)), d(nk)
    gs, gi = m.grid_build(dk, dn, M.FUSE_GRID)
    qm, qdist, nf = [to_host(x) for x in m.Fuse(dk, d(desc), dn, gs, gi, _query_bytes(qs, backend), d(qd), d(nq), M.FUSE_GRID, inv_sigma2, d(ur),
                                                 th_dist=th)]
    for b, (fr, q, qdesc, exp, n) in enumerate(entries):
        wm = np.array([-1 if lab < 0 else fr["index"][lab] for lab, _ in exp[:n]], np.int32).reshape(-1)
        wd = np.array([dist for _, dist in exp[:n]], np.int32).reshape(-1)
        om, od, on = O.fuse(fr["kps"], fr["desc"], q[:n], qdesc[:n], M.FUSE_GRID, th, inv_sigma2, fr["u_right"])
        if n == 0:
            om, od = om[:0], od[:0]
        three_way(qm[b, :n], om, wm, "entry %d bestIdx" % b)
        three_way(qdist[b, :n], od, wd, "entry %d bestDist" % b)
        three_way(nf[b], on, int((wm >= 0).sum()), "entry %d nFused" % b)
        assert (qm[b, n:] == -1).all(), "entry %d: a query behind nq was searched" % b


@pytest.mark.parametrize("backend", BACKENDS)
def test_fuse_windows_chunks_borders(lib, backend):
    """Windows of 65, 128 and 200 entries; best in the second and third chunk; equal distances across chunk boundaries (first in the
    enumeration order ix outer, iy inner, index order in a cell; index order runs the other way); |dx| == r and |dy| == r; dist ==
    th_dist and th_dist + 1; the level filter; windows clamped at the four borders and wholly outside; Q_VALID cleared; cap_q % 4 != 0;
    nq = 0."""
    e0, e1, e2 = cached(M.fuse_case, 61, 0), cached(M.fuse_case, 62, 5), cached(M.fuse_case, 63, 2)
    _fuse_check(lib, backend, [e0 + (len(e0[1]),), e1 + (len(e1[1]) - 3,), e2 + (0,)], TH_LOW, None)


@pytest.mark.parametrize("backend", BACKENDS)
def test_fuse_chi2_gate(lib, backend):
    """the reprojection gate with monocular and stereo key points (u_right of -1, 0.0 and positive), at levels 0 and 1"""
    es = [cached(M.fuse_chi2_case, s) for s in (64, 65, 66)]
    big = cached(M.fuse_case, 63, 2)      # a larger frame, so that the gate entries leave slack; its queries are not asked (nq = 0)
    _fuse_check(lib, backend, [es[0][:4] + (len(es[0][1]),), es[1][:4] + (len(es[1][1]) - 2,), big + (0,)], TH_LOW, es[0][4])


@pytest.mark.parametrize("backend", BACKENDS)
def test_search_by_sim3(lib, backend):
    """mutual pairs, one-directional pairs, invalid queries on either side, distance 100 = TH_HIGH and 101; a full, a partly filled and
    an empty entry"""
    built = [cached(M.sim3_case, 71, 0), cached(M.sim3_case, 72, 4), cached(M.sim3_case, 73, 1)]
    empty = [False, False, True]
    B = len(built)
    m = orbhip.ORBmatcher(lib=lib)
    d = lambda a: to_dev_plain(a, backend)   # noqa: E731
    sides, qs = [], []
    for w in (0, 1):
        fr = [c[w] for c in built]
        cap = max(f["n"] for f in fr)
        q, qdsc = [c[2 + 2 * w] for c in built], [c[3 + 2 * w] for c in built]
        kps = M.pack_rows([f["kps"] for f in fr], cap, [f["kps"] for f in fr]).view(np.float32).reshape(B, cap, 7)
        n = d(np.array([0 if e else f["n"] for f, e in zip(fr, empty)], np.int32))
        dk = d(kps)
        gs, gi = m.grid_build(dk, n, M.FUSE_GRID)
        sides.append(dict(kps=dk, desc=d(M.pack_rows([f["desc"] for f in fr], cap, [f["desc"] for f in fr])), counts=n, grid_start=gs, grid_idx=gi,
                          grid=M.FUSE_GRID))
        qs.append((_query_bytes(M.pack_rows(q, cap, q), backend), d(M.pack_rows(qdsc, cap, qdsc))))
    got, cnt = [to_host(x) for x in m.SearchBySim3(sides[0], sides[1], qs[0][0], qs[0][1], qs[1][0], qs[1][1])]
    for b, (f1, f2, q12, q12d, q21, q21d, exp) in enumerate(built):
        if empty[b]:
            assert cnt[b] == 0 and (got[b] == -1).all()
            continue
        want, n = M.expect_array(exp, f1, f2, by_dst=False)
        om, on = O.search_by_sim3(f1["kps"], f1["desc"], M.FUSE_GRID, f2["kps"], f2["desc"], M.FUSE_GRID, q12, q12d, q21, q21d)
        three_way(got[b, :f1["n"]], om, want, "entry %d vpMatches12" % b)
        three_way(cnt[b], on, n, "entry %d nFound" % b)
        assert (got[b, f1["n"]:] == -1).all()


def _agreement(m12, m21, n1, n2):
    """ORBmatcher.cc:2213-2219 in plain Python"""
    out = np.full(len(m12), -1, np.int32)
    for i1 in range(n1):
        idx2 = m12[i1]
        if 0 <= idx2 < n2 and m21[idx2] == i1:
            out[i1] = idx2
    return out, int((out >= 0).sum())


@pytest.mark.parametrize("backend", BACKENDS)
def test_mutual_matches(lib, backend):
    """cap1 = 300 with n1 = 257; m12 entries >= n2 whose slack entry agrees; i1 >= n1 whose lists agree; one-directional pairs; the same
    lists with full counts (the slack pairs then count) and with n1 = 0"""
    m12, m21, n1, n2, exp, n = M.mutual_case()
    full = exp.copy()
    full[[100, 101, 257, 299]] = [30, 39, 9, 10]       # with n1 = cap1 and n2 = cap2 the four pairs behind the counts agree too
    a12 = np.stack([m12, m12, m12[::-1]]); a21 = np.stack([m21, m21, m21[::-1]])    # entry 1: counts at capacity; entry 2: n1 = 0
    n1v, n2v = np.array([n1, 300, 0], np.int32), np.array([n2, 40, n2], np.int32)
    wants = [(exp, n), (full, n + 4), (np.full(300, -1, np.int32), 0)]
    d = lambda a: to_dev_plain(a, backend)   # noqa: E731
    d12, d21, dn1, dn2 = d(a12), d(a21), d(n1v), d(n2v)
    out, nf = zeros(d12, (3, 300), np.int32), zeros(d12, (3,), np.int32)
    check(lib.orbm_mutual_matches(ptr(d12), ptr(d21), ptr(dn1), ptr(dn2), 300, 40, 3, ptr(out), ptr(nf), stream(d12)), "orbm_mutual_matches")
    out, nf = to_host(out), to_host(nf)
    for b, (want, cnt) in enumerate(wants):
        ref = _agreement(a12[b], a21[b], int(n1v[b]), int(n2v[b]))
        three_way(out[b], ref[0], want, "entry %d" % b)
        three_way(nf[b], ref[1], cnt, "entry %d count" % b)


# ---- SearchForInitialization -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_search_for_initialization(lib, backend):
    """The steal chain (A at 20, B takes it at 10, C at exactly 10 is refused); level1 > 0 ignored; the ratio boundary; a stolen feature's
    stale histogram entry culled without a second decrement; vbPrevMatched updated only for the final matches; a second call from the first
    call's vbPrevMatched that finds a better match."""
    built = [cached(M.init_case, 81, 0), cached(M.init_case, 82, 5), cached(M.init_case, 83, 2)]
    empty = [False, False, True]
    B = len(built)
    c1, c2 = max(len(c["k1"]) for c in built), max(len(c["k2"]) for c in built)
    assert c1 <= 40 and c2 <= 40
    d = lambda a: to_dev_plain(a, backend)   # noqa: E731
    # traps behind n1: level-0 features with F2's descriptors, looking at F2's first key point
    k1 = M.pack_rows([c["k1"] for c in built], c1, [c["k2"][:1] for c in built]).view(np.float32).reshape(B, c1, 7)
    d1 = M.pack_rows([c["d1"] for c in built], c1, [c["d2"][:1] for c in built])
    k2 = M.pack_rows([c["k2"] for c in built], c2, [c["k2"] for c in built]).view(np.float32).reshape(B, c2, 7)
    d2 = M.pack_rows([c["d2"] for c in built], c2, [c["d1"] for c in built])
    prev0 = M.pack_rows([c["prev0"] for c in built], c1, [np.stack([c["k2"]["x"][:1], c["k2"]["y"][:1]], 1) for c in built])
    n1 = np.array([0 if e else len(c["k1"]) for c, e in zip(built, empty)], np.int32)
    n2 = np.array([0 if e else len(c["k2"]) for c, e in zip(built, empty)], np.int32)
    m = orbhip.ORBmatcher(0.9, True, lib=lib)
    dk1, dd1, dn1, dk2, dd2, dn2, prev = d(k1), d(d1), d(n1), d(k2), d(d2), d(n2), d(prev0.copy())
    gs, gi = m.grid_build(dk2, dn2, M.FUSE_GRID)
    oprev = [c["prev0"] for c in built]
    for call in range(2):
        qm, nm = [to_host(x) for x in m.SearchForInitialization(dk1, dd1, dn1, dk2, dd2, dn2, gs, gi, prev, M.FUSE_GRID, 20)]
        ph = to_host(prev)
        for b, c in enumerate(built):
            nb = len(c["k1"])
            if empty[b]:
                assert nm[b] == 0 and (qm[b] == -1).all() and np.array_equal(ph[b], prev0[b])
                continue
            w = c["calls"][call]
            om, on, oprev[b] = O.search_for_initialization(c["k1"], c["d1"], c["k2"], c["d2"], M.FUSE_GRID, oprev[b], 20, 0.9, True)
            three_way(qm[b, :nb], om, w["match"], "call %d entry %d vnMatches12" % (call, b))
            three_way(nm[b], on, w["n"], "call %d entry %d nmatches" % (call, b))
            three_way(ph[b, :nb], oprev[b], w["prev"], "call %d entry %d vbPrevMatched" % (call, b))
            assert (qm[b, nb:] == -1).all() and np.array_equal(ph[b, nb:], prev0[b, nb:]), "entry %d: a slack feature was searched" % b
    assert not np.array_equal(built[0]["calls"][0]["match"], built[0]["calls"][1]["match"])   # the second call really differs


# ---- DescriptorDistance / knnMatch2 against np.unpackbits -----------------------------------------------------------------------------
def _dist(q, t):
    return np.unpackbits(q[:, None, :] ^ t[None, :, :], axis=-1).sum(-1).astype(np.int64)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("nt", [1, 255, 256, 257])
@pytest.mark.parametrize("nq", [1, 15, 16, 17])
def test_descriptor_distance_shapes(lib, backend, nq, nt):
    rng = np.random.default_rng(1000 * nq + nt)
    B = 3
    q = rng.integers(0, 256, (B, nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (B, nt, 32), dtype=np.uint8)
    t[1, nt - 1] = q[1, nq - 1]; t[2, 0] = ~q[2, 0]                   # a distance of 0 and one of 256 at the corners
    D = to_host(orbhip.ORBmatcher(lib=lib).DescriptorDistance(to_dev_plain(q, backend), to_dev_plain(t, backend)))
    D = D.view(np.uint16) if D.dtype == np.int16 else D
    for b in range(B):
        same(D[b].astype(np.int64), _dist(q[b], t[b]), "entry %d" % b)
    assert D[1, nq - 1, nt - 1] == 0 and D[2, 0, 0] == 256


def _knn2_ref(q, t):
    """the two nearest trains per query, the lower index first among equals (stable sort); -1 / 256 where there are fewer than two"""
    idx = np.full((len(q), 2), -1, np.int32); dist = np.full((len(q), 2), 256, np.int32)
    if len(t) and len(q):
        D = _dist(q, t)
        order = np.argsort(D, axis=1, kind="stable")[:, :2]
        k = order.shape[1]
        idx[:, :k] = order
        dist[:, :k] = np.take_along_axis(D, order, 1)
    return idx, dist


def _knn2_check(lib, backend, nqs, nts, cap_q, cap_t, seed):
    rng = np.random.default_rng(seed)
    B = len(nqs)
    q = rng.integers(0, 256, (B, cap_q, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (B, cap_t, 32), dtype=np.uint8)
    for b in range(B):
        if nts[b] >= 65 and nqs[b] > 0:          # equal descriptors at train indices 63 and 64, equal to the last query
            t[b, 63] = t[b, 64] = q[b, nqs[b] - 1]
        t[b, nts[b]:] = q[b, np.arange(cap_t - nts[b]) % cap_q]      # traps behind nt: copies of the queries (distance 0)
    m = orbhip.ORBmatcher(lib=lib)
    d = lambda a: to_dev_plain(a, backend)   # noqa: E731
    idx, dist = [to_host(x) for x in m.knnMatch2(d(q), d(np.array(nqs, np.int32)), d(t), d(np.array(nts, np.int32)))]
    for b in range(B):
        ri, rd = _knn2_ref(q[b, :nqs[b]], t[b, :nts[b]])
        same(idx[b, :nqs[b]], ri, "entry %d (nq %d, nt %d) indices" % (b, nqs[b], nts[b]))
        same(dist[b, :nqs[b]], rd, "entry %d distances" % b)
        if nts[b] >= 65 and nqs[b] > 0:
            assert idx[b, nqs[b] - 1].tolist() == [63, 64] and dist[b, nqs[b] - 1].tolist() == [0, 0], "entry %d: equal trains 63 and 64" % b
    for b in range(B):
        assert (idx[b, nqs[b]:] == -1).all() and (dist[b, nqs[b]:] == 256).all(), "entry %d: rows behind nq" % b


@pytest.mark.parametrize("backend", BACKENDS)
def test_knn2_query_counts(lib, backend):
    """nq in {1, 255, 256, 257, 600} (one, two and three workgroups), ragged, with 65 to 129 trains"""
    _knn2_check(lib, backend, [1, 255, 256, 257, 600, 0], [129, 65, 66, 65, 65, 65], 603, 130, 5)


@pytest.mark.parametrize("backend", BACKENDS)
def test_knn2_train_counts(lib, backend):
    """nt in {0, 1, 2, 63, 64, 65, 129} (tiles of 64), ragged query counts"""
    _knn2_check(lib, backend, [70, 3, 257, 64, 65, 70, 258], [0, 1, 2, 63, 64, 65, 129], 258, 131, 6)
