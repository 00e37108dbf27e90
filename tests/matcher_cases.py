"""Constructed inputs for the mapping-side matcher kernels (tests/test_matcher_constructed.py): plain numpy, no extractor.

Every builder states the outcome the reference's text prescribes for its case as a literal in the builder (feature *labels*; the random
renumbering of a seed turns them into indices), next to the inputs.  Nothing here calls the code under test or the oracle.

Descriptors carry exact distances: a "track" is a random 256-bit base; a member of a track is the base with k bits flipped that no other
member of the track flips, so the distance between two members is the sum of their k.  Members of different tracks are "unrelated" and at
least MIN_UNRELATED apart (a condition of the generator, asserted for the fixed seeds used; not a tolerance)."""
import numpy as np

from orbhip._lib import KP_DTYPE
from orbhip.matcher import Q_VALID, QUERY_DTYPE, TRI_KB8_PAIR_DTYPE, TRI_PAIR_DTYPE

MIN_UNRELATED = 80
NODE_SIZES = (1, 2, 63, 64, 65, 130)           # sizes of the inner side's shared nodes
BEST_POS = {1: 0, 2: 1, 63: 0, 64: 63, 65: 64, 130: 129}   # where the best candidate sits in a node of that size
TRAP_NODE = 100000                             # a node id behind every real one
_POP = np.array([bin(i).count("1") for i in range(256)], np.uint16)


def hamming_matrix(a, b):
    """[len(a), len(b)] Hamming distances of 32-byte descriptors, by table look-up"""
    return _POP[a[:, None, :] ^ b[None, :, :]].sum(-1).astype(np.int32)


class Pool:
    """the descriptors of one case: rows of tracks with exact mutual distances"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.base, self.free, self.rows, self.track = [], [], [], []

    def new_track(self):
        self.base.append(self.rng.integers(0, 2, 256).astype(np.uint8))
        self.free.append(list(self.rng.permutation(256)))
        return len(self.base) - 1

    def member(self, t, k):
        """a row at distance k from the base of track t (k fresh bit positions) -> row number"""
        bits = self.base[t].copy()
        for _ in range(k):
            bits[self.free[t].pop()] ^= 1
        self.rows.append(np.packbits(bits, bitorder="little"))
        self.track.append(t)
        return len(self.rows) - 1

    def base_row(self):
        """a new track's base -> (track, row)"""
        t = self.new_track()
        return t, self.member(t, 0)

    def filler(self):
        return self.base_row()[1]

    def array(self):
        d = np.array(self.rows, np.uint8).reshape(-1, 32)
        t = np.array(self.track)
        D = hamming_matrix(d, d)
        unrelated = t[:, None] != t[None, :]
        assert not unrelated.any() or D[unrelated].min() >= MIN_UNRELATED, "pick another seed: unrelated descriptors closer than %d" % MIN_UNRELATED
        return d


def keypoint(x=0.0, y=0.0, octave=0, angle=0.0):
    k = np.zeros((), KP_DTYPE)
    k["x"], k["y"], k["octave"], k["angle"], k["size"], k["response"], k["class_id"] = x, y, octave, angle, 31, 40, -1
    return k


class Side:
    """one key frame / frame of a FeatureVector search: features are added node by node, in the order they stand inside the node"""

    def __init__(self):
        self.f = []

    def add(self, row, node, valid=1, angle=0.0, right=False, x=0.0, y=0.0, octave=0, ur=-1.0, has_mp=0):
        self.f.append(dict(row=row, node=node, valid=valid, angle=angle, right=right, x=x, y=y, octave=octave, ur=ur, has_mp=has_mp))
        return len(self.f) - 1      # the feature's label

    def finish(self, desc, rng, n_left=None):
        """labels -> feature indices by a random renumbering (left-camera features first on a rig), then the CSR: node ids ascending,
        feat_idx in the order of adding.  n_left: None (one camera), "split" (right=True features are >= n_left), "all" or "none"."""
        n = len(self.f)
        right = np.array([f["right"] for f in self.f], bool) if n_left == "split" else np.zeros(n, bool)
        index = np.zeros(n, np.int64)
        nl = int((~right).sum())
        index[~right] = rng.permutation(nl)
        index[right] = nl + rng.permutation(n - nl)
        o = dict(desc=np.zeros((n, 32), np.uint8), angle=np.zeros(n, np.float32), valid=np.zeros(n, np.uint8), kps=np.zeros(n, KP_DTYPE),
                 u_right=np.zeros(n, np.float32), has_mp=np.zeros(n, np.uint8), index=index, n=n,
                 n_left={None: -1, "split": nl, "all": n, "none": 0}[n_left])
        for f, i in zip(self.f, index):
            o["desc"][i], o["angle"][i], o["valid"][i], o["u_right"][i], o["has_mp"][i] = desc[f["row"]], f["angle"], f["valid"], f["ur"], f["has_mp"]
            o["kps"][i] = keypoint(f["x"], f["y"], f["octave"], f["angle"])
        ids = sorted({f["node"] for f in self.f})
        start, feat = [0], []
        for nid in ids:
            feat += [int(index[lab]) for lab, f in enumerate(self.f) if f["node"] == nid]
            start.append(len(feat))
        o.update(node_id=np.array(ids, np.int32), node_start=np.array(start, np.int32), feat_idx=np.array(feat, np.int32), n_nodes=len(ids))
        return o


def expect_array(pairs, src, dst, by_dst):
    """label pairs {outer label: inner label} -> (index array, count): by_dst: out[inner index] = outer index (SearchByBoW(KF,F)),
    else out[outer index] = inner index"""
    out = np.full(dst["n"] if by_dst else src["n"], -1, np.int32)
    for a, b in pairs.items():
        if by_dst:
            out[dst["index"][b]] = src["index"][a]
        else:
            out[src["index"][a]] = dst["index"][b]
    return out, len(pairs)


def oracle_side(s):
    """what tests/oracle_lib takes for one side"""
    return dict(desc=s["desc"], angle=s["angle"], kps=s["kps"], u_right=s["u_right"], has_mp=s["has_mp"], node_id=s["node_id"],
                node_start=s["node_start"], feat_idx=s["feat_idx"], n_nodes=s["n_nodes"])


# ---- the slab packer --------------------------------------------------------------------------------------------------------------
def pack_rows(rows, cap, trap=None, dtype=None):
    """per-entry arrays [n_b, ...] -> [B, cap, ...]; the slack behind n_b is filled with the entry's trap rows, cycled (zeros without)"""
    first = np.asarray(rows[0])
    out = np.zeros((len(rows), cap) + first.shape[1:], dtype or first.dtype)
    for b, r in enumerate(rows):
        n = len(r)
        assert n <= cap
        out[b, :n] = r
        t = None if trap is None else trap[b]
        if t is not None and len(t) and n < cap:
            out[b, n:] = np.asarray(t)[np.arange(cap - n) % len(t)]
    return out


def pack_sides(entries, others, cap_f, cap_n, trap_node_of=None):
    """B sides -> the slabs of one orbm_bow_side / orbm_tri_side, ragged: entry b holds entries[b]["n"] features and n_nodes nodes.  An
    entry marked empty=True keeps all its data but counts n_nodes = 0.  The slack features behind n are traps: valid, without a map point,
    with the descriptors (and key points) of the OTHER side's features, reachable through a trap node behind n_nodes whose id is
    trap_node_of(b) (default TRAP_NODE): a walk past n_nodes or past n wins a match."""
    B = len(entries)

    def trap_rows(b, what):   # the other side's features of the node whose id the trap node takes (all of them for TRAP_NODE)
        o = others[b]
        ids = list(o["node_id"])
        if trap_node_of and trap_node_of(b) in ids:
            k = ids.index(trap_node_of(b))
            return o[what][o["feat_idx"][o["node_start"][k]:o["node_start"][k + 1]]]
        return o[what]
    trap_d = [trap_rows(b, "desc") for b in range(B)]
    trap_k = [trap_rows(b, "kps") for b in range(B)]
    out = dict(desc=pack_rows([e["desc"] for e in entries], cap_f, trap_d), angle=pack_rows([e["angle"] for e in entries], cap_f),
               valid=pack_rows([e["valid"] for e in entries], cap_f, [np.ones(1, np.uint8)] * B),
               has_mp=pack_rows([e["has_mp"] for e in entries], cap_f), u_right=pack_rows([e["u_right"] for e in entries], cap_f, [np.full(1, -1, np.float32)] * B),
               kps=pack_rows([e["kps"] for e in entries], cap_f, trap_k).view(np.float32).reshape(B, cap_f, 7),
               node_id=np.zeros((B, cap_n), np.int32), node_start=np.zeros((B, cap_n + 1), np.int32), feat_idx=np.zeros((B, cap_f), np.int32),
               n_nodes=np.zeros(B, np.int32), n_left=np.array([e["n_left"] for e in entries], np.int32))
    for b, e in enumerate(entries):
        n, nn = e["n"], e["n_nodes"]
        assert nn <= cap_n and n <= cap_f
        out["node_id"][b, :nn] = e["node_id"]
        out["node_start"][b, :nn + 1] = e["node_start"]
        out["feat_idx"][b, :n] = e["feat_idx"]
        out["feat_idx"][b, n:] = np.arange(n, cap_f)                        # the slack features, in one trap node
        first = trap_node_of(b) if trap_node_of else TRAP_NODE
        assert nn == 0 or first > e["node_id"][-1]
        out["node_id"][b, nn:] = first + np.arange(cap_n - nn)
        out["node_start"][b, nn + 1:] = cap_f
        out["n_nodes"][b] = 0 if e.get("empty") else nn
    return out


def as_empty(e):
    return dict(e, empty=True)


# ---- SearchByBoW ------------------------------------------------------------------------------------------------------------------
BOW_RATIO = 0.9     # with it an unrelated second-best (>= 80) never fails the ratio test of a best <= 51: 51 < 0.9f * 80 = 72
BACK_NODE = 95      # the inner side's node behind every node of the outer side


def bow_main_case(seed, kk, pad=0):
    """Both overloads at mfNNratio = BOW_RATIO.  kk: SearchByBoW(KeyFrame, KeyFrame), whose inner side has validity flags and whose
    acceptance is bestDist1 < TH_LOW (ORBmatcher.cc:1067) where SearchByBoW(KeyFrame, Frame) has <= TH_LOW (:464).
    -> (outer Side data, inner Side data, expected {outer label: inner label})"""
    P = Pool(seed)
    A, Bs = Side(), Side()          # outer (the key frame whose features are walked), inner
    exp = {}

    def pair(node, k, size=1, pos=0, **kw):
        """one outer feature in `node`; the inner node has `size` features, the one at `pos` at distance k, unrelated ones elsewhere"""
        t, r = P.base_row()
        a = A.add(r, node, **kw)
        lab = None
        for p in range(size):
            x = Bs.add(P.member(t, k) if p == pos else P.filler(), node)
            lab = x if p == pos else lab
        return a, lab, t

    # nodes on one side only, at the front, in the middle and at the back of the id lists; the outer-only node 25 and the inner-only node
    # 26 hold the same descriptor, as do 1 / 2 and 90 / BACK_NODE: pairing nodes by position instead of by id matches them
    for na, nb in ((1, 2), (25, 26), (90, BACK_NODE)):
        t, r = P.base_row()
        A.add(r, na)
        Bs.add(P.member(t, 0), nb)
    # inner node sizes 1, 2, 63, 64, 65, 130 with the best candidate (distance 15) at position 0, 1, 0, 63, 64, 129: all matched.
    # The node of 130 serves three more outer features (a node holds several tracks; they are unrelated to each other):
    #   equal best candidates (12, 12) at positions 3 and 70, in different 64-entry chunks: the first is bestIdx, the second becomes
    #   bestDist2 = bestDist1, and 12 < 0.9 * 12 fails: no match
    #   (14, 12) at positions 4 and 71: 12 < 0.9f * 14 = 12.6 -> position 71.        (13, 12) at positions 5 and 72: 12 < 11.7 fails
    for j, size in enumerate(NODE_SIZES):
        node = 10 + j
        t, r = P.base_row()
        a = A.add(r, node)
        planted, ties = {BEST_POS[size]: (t, 15)}, []
        if size == 130:
            for off, (k_first, k_second, want) in enumerate(((12, 12, None), (14, 12, 71), (13, 12, None))):
                tt, rr = P.base_row()
                ties.append((A.add(rr, node), want))
                planted[3 + off], planted[70 + off] = (tt, k_first), (tt, k_second)
        labs = [Bs.add(P.member(*planted[p]) if p in planted else P.filler(), node) for p in range(size)]
        exp[a] = labs[BEST_POS[size]]
        for aa, want in ties:
            if want is not None:
                exp[aa] = labs[want]
    # best distance 49, 50, 51 alone in its node (bestDist2 = 256): 49 both, 50 only (KF,F), 51 neither
    a, b, _ = pair(20, 49); exp[a] = b
    a, b, _ = pair(21, 50)
    if not kk:
        exp[a] = b
    pair(22, 51)
    # node 40: outer a0 (the base) and a1 (2 bits off) share the best inner feature i1 (10 bits off): a0 takes it (10 < 0.9 * 30), a1 must
    # see it as taken (vpMapPointMatches[realIdxF] / vbMatched2) and takes i2 (30 bits off, distance 32, alone -> bestDist2 = 256)
    t, r = P.base_row()
    a0, a1 = A.add(r, 40), A.add(P.member(t, 2), 40)
    i1, i2 = Bs.add(P.member(t, 10), 40), Bs.add(P.member(t, 30), 40)
    exp[a0], exp[a1] = i1, i2
    # node 41: an outer feature without a good map point facing a perfect candidate: skipped
    pair(41, 0, valid=0)
    # node 42: the nearest inner feature (5) is invalid.  (KF,KF) skips it and takes the one at 25; (KF,F) has no inner validity: 5 < 0.9 * 25
    t, r = P.base_row()
    a = A.add(r, 42)
    j5, j25 = Bs.add(P.member(t, 5), 42, valid=0), Bs.add(P.member(t, 25), 42)
    exp[a] = j25 if kk else j5
    # node 43: 65 outer features against 2 inner ones; only the last outer feature is related (20) and matches
    for _ in range(64):
        A.add(P.filler(), 43)
    t, r = P.base_row()
    a = A.add(r, 43)
    Bs.add(P.filler(), 43)
    exp[a] = Bs.add(P.member(t, 20), 43)
    for _ in range(pad):            # unrelated features in an outer-only / inner-only node: they fill an entry up to its capacity
        A.add(P.filler(), 50)
        Bs.add(P.filler(), 51)
    d = P.array()
    return A.finish(d, P.rng), Bs.finish(d, P.rng), exp


def bow_ratio_case(seed, ratio, kk):
    """The ratio test `(float)bestDist1 < mfNNratio * (float)bestDist2` (:470 / :1069) on its float boundary, nodes of two inner features.
    0.6f * 50.0f rounds UP to 30.000002f, so (30, 50) passes at ratio 0.6 and (31, 50) is the first to fail; 0.5f * 50.0f = 25 exactly, so
    (25, 50) fails and (24, 50) passes.  (KF,KF) refuses nothing here by TH_LOW: every best is < 50."""
    P = Pool(seed)
    A, Bs = Side(), Side()
    exp = {}
    accepted = {0.6: {(29, 50): True, (30, 50): True, (31, 50): False}, 0.5: {(24, 50): True, (25, 50): False, (26, 50): False}}[ratio]
    for node, ((k1, k2), ok) in enumerate(accepted.items()):
        t, r = P.base_row()
        a = A.add(r, node)
        far, near = Bs.add(P.member(t, k2), node), Bs.add(P.member(t, k1), node)
        if ok:
            exp[a] = near
    d = P.array()
    return A.finish(d, P.rng), Bs.finish(d, P.rng), exp


def bow_rig_case(seed, n_left):
    """SearchByBoW(KeyFrame, Frame) with F.Nleft != -1 (:429-457, :513-542) at ratio 0.9.  Inner features are added as left (L) or right (R)
    camera features.  n_left = "split": R features get indices >= Nleft;  "all": Nleft = N, every feature is a left one;  "none": Nleft = 0,
    every feature is a right one, bestDist1 stays 256 and nothing is matched.  -> (outer, inner, expected LIST of (outer, inner) label pairs)"""
    P = Pool(seed)
    A, Bs = Side(), Side()
    spec = [  # per node: the inner features as (camera, distance)
        [("L", 10), ("R", 20)],             # 0
        [("L", 30), ("L", 31), ("R", 45)],  # 1
        [("L", 51), ("R", 5)],              # 2
        [("R", 5)],                         # 3
        [("L", 10), ("R", 51)],             # 4
        [("L", 10), ("R", 8), ("R", 8)],    # 5
    ]
    labs = []
    for node, cands in enumerate(spec):
        t, r = P.base_row()
        a = A.add(r, node)
        labs.append((a, [Bs.add(P.member(t, k), node, right=(cam == "R")) for cam, k in cands]))
    nL = sum(c == "L" for cands in spec for c, _ in cands)
    nR = sum(c == "R" for cands in spec for c, _ in cands)
    for _ in range(nR - nL):                # Nleft = N / 2 for "split"
        Bs.add(P.filler(), 9, right=False)
    want = {
        # split: 0: left 10 (10 < 0.9 * 256) and right 20 ride along.  1: left 30 < 0.9f * 31 = 27.9 fails, the right one at 45 <= TH_LOW is
        # still taken (the right camera's ratio test is `|| true`, :515).  2: left best 51 > TH_LOW: neither.  3: no left candidate, bestDist1
        # = 256: neither.  4: left only (right 51 > TH_LOW).  5: left 10, and the FIRST of the two equal right ones
        "split": [(0, 0), (0, 1), (1, 2), (4, 0), (5, 0), (5, 1)],
        # all: one camera.  0: 10 < 0.9 * 20.  1: 30 < 27.9 fails.  2: 5 < 0.9 * 51.  3: 5 alone.  4: 10 < 0.9 * 51.  5: 8 < 0.9 * 8 fails
        "all": [(0, 0), (2, 1), (3, 0), (4, 0)],
        "none": [],
    }[n_left]
    d = P.array()
    return A.finish(d, P.rng), Bs.finish(d, P.rng, n_left), [(labs[n][0], labs[n][1][j]) for n, j in want]


def bow_rotation_case(seed):
    """13 matches (each alone in its node, distance 10) whose rotation differences rot = angle1 - angle2 fall, with factor 1 / HISTO_LENGTH
    (:344), into bin round(rot / 30): ten in bin 0, one each in bins 2, 5, 7 (rot 60, 150, 210) and one with a negative difference (10 - 40
    -> 330 -> bin 11).  ComputeThreeMaxima (:2654-2695) takes strictly larger counts only, so of the equal bins 2, 5, 7, 11 the first two
    become ind2, ind3; max2 = 1 is exactly 0.1f * 10 and `max2 < 0.1f * max1` is false, so they stay.  Bins 7 and 11 are culled.
    -> (outer, inner, expected with orientation check, expected without)"""
    P = Pool(seed)
    A, Bs = Side(), Side()
    on, off = {}, {}
    angles = [(0.0, 0.0)] * 10 + [(60.0, 0.0), (150.0, 0.0), (210.0, 0.0), (10.0, 40.0)]
    for node, (a1, a2) in enumerate(angles):
        t, r = P.base_row()
        a, b = A.add(r, node, angle=a1), Bs.add(P.member(t, 10), node, angle=a2)
        off[a] = b
        if node < 12:
            on[a] = b
    d = P.array()
    return A.finish(d, P.rng), Bs.finish(d, P.rng), on, off


# ---- SearchForTriangulation (pinhole) -----------------------------------------------------------------------------------------------
# F12 with F[5] = -1, F[7] = 1 (row major): the epipolar line of kp1 in image 2 is (a, b, c) = (0, 1, -y1), den = 1 and the gate of
# Pinhole::epipolarConstrain reads (y2 - y1)^2 < 3.84 * sigma2[octave2].  sigma2 = scale^2 with scale 1.2^level: level 0 passes dy = 1
# (1 < 3.84) and fails dy = 3.
TRI_F12 = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)
TRI_EP = np.array([1000.0, 1000.0], np.float32)
TRI_SCALE = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
TRI_SIGMA2 = (TRI_SCALE * TRI_SCALE).astype(np.float32)


def tri_case(seed, pad=0):
    """-> (KF1 side, KF2 side, expected dict of {KF1 label: KF2 label} for the modes "plain", "coarse", "only_stereo", "f0" (F12 = 0, den
    == 0: no candidate passes), "f0_coarse" (= "coarse": bCoarse short-circuits the gate, ORBmatcher.cc:1347) and "kb8_coarse" (one
    KannalaBrandt8 camera per key frame, bCoarse).
    Every key point sits far from the epipole (1000, 1000) unless its case says otherwise; y1 = y2 = 50 passes the epipolar gate."""
    P = Pool(seed)
    A, Bs = Side(), Side()
    plain, coarse, stereo, no_u_right = {}, {}, {}, []
    both = lambda a, b: (plain.__setitem__(a, b), coarse.__setitem__(a, b))   # noqa: E731
    Y = 50.0
    # KF2 node sizes with the best candidate (15) at the listed position.  The node of 130 serves a second KF1 feature with equal distances
    # (12) at positions 3 and 70: the LAST one wins (`dist > bestDist -> continue`, :1290)
    for j, size in enumerate(NODE_SIZES):
        t, r = P.base_row()
        a = A.add(r, 10 + j, x=10.0 * j, y=Y)
        planted = {BEST_POS[size]: (t, 15)}
        if size == 130:
            tt, rr = P.base_row()
            a_tie = A.add(rr, 10 + j, x=5.0, y=Y)
            planted[3], planted[70] = (tt, 12), (tt, 12)
        labs = [Bs.add(P.member(*planted[p]) if p in planted else P.filler(), 10 + j, x=float(p), y=Y) for p in range(size)]
        both(a, labs[BEST_POS[size]])
        if size == 130:
            both(a_tie, labs[70])
    # node 21: the nearest candidate (5) fails the epipolar gate (dy = 3), the next one (20) is taken; bCoarse takes the nearest
    t, r = P.base_row()
    a = A.add(r, 21, x=5.0, y=Y)
    c5, c20 = Bs.add(P.member(t, 5), 21, x=6.0, y=Y + 3), Bs.add(P.member(t, 20), 21, x=7.0, y=Y)
    plain[a], coarse[a] = c20, c5
    # node 22: equal distances (12); the later one fails the gate, so the earlier one is kept; bCoarse takes the later one
    t, r = P.base_row()
    a = A.add(r, 22, x=5.0, y=Y)
    e0, e1 = Bs.add(P.member(t, 12), 22, x=6.0, y=Y), Bs.add(P.member(t, 12), 22, x=7.0, y=Y + 3)
    plain[a], coarse[a] = e0, e1
    # node 23: two KF1 features pick the same KF2 feature (10 and 12); vbMatched2 is never set, both keep it
    t, r = P.base_row()
    a0, a1 = A.add(r, 23, x=5.0, y=Y), A.add(P.member(t, 2), 23, x=6.0, y=Y)
    i = Bs.add(P.member(t, 10), 23, x=8.0, y=Y)
    both(a0, i); both(a1, i)
    # nodes 30-33: distance^2 to the epipole against 100 * mvScaleFactors[octave] (:1307): level 0: 6^2 + 8^2 = 100 is not < 100 -> kept;
    # 6^2 + 7^2 = 85 -> dropped.  level 1: 100 * 1.2f = 120.00001: 9^2 + 6^2 = 117 -> dropped (kept at level 0); 11^2 = 121 -> kept
    for node, (dx, dy, octv, keep) in enumerate(((6, 8, 0, True), (6, 7, 0, False), (9, 6, 1, False), (11, 0, 1, True)), 30):
        t, r = P.base_row()
        a = A.add(r, node, x=1.0, y=1000.0 + dy)
        b = Bs.add(P.member(t, 10), node, x=1000.0 + dx, y=1000.0 + dy, octave=octv)
        if keep:
            both(a, b)
    # nodes 40-44: mvuRight >= 0 counts as stereo, 0.0 included; the candidate sits 85 from the epipole and only two monocular features
    # take the epipole test (:1301).  bOnlyStereo wants both sides stereo (:1244, :1280)
    for node, (ur1, ur2, keep) in enumerate(((-1.0, -1.0, False), (0.0, -1.0, True), (-1.0, 0.0, True), (-1.0, 5.0, True), (0.0, 3.0, True)), 40):
        t, r = P.base_row()
        a = A.add(r, node, x=1.0, y=1007.0, ur=ur1)
        b = Bs.add(P.member(t, 10), node, x=1006.0, y=1007.0, ur=ur2)
        if keep:
            both(a, b)
        if ur1 >= 0 and ur2 >= 0:
            stereo[a] = b
        no_u_right.append(a)
    # node 50: the KF1 feature holds a map point: skipped.  node 51: the nearest KF2 feature (5) holds one, the next (25) is taken
    t, r = P.base_row()
    A.add(r, 50, x=5.0, y=Y, has_mp=1)
    Bs.add(P.member(t, 0), 50, x=6.0, y=Y)
    t, r = P.base_row()
    a = A.add(r, 51, x=5.0, y=Y)
    Bs.add(P.member(t, 5), 51, x=6.0, y=Y, has_mp=1)
    both(a, Bs.add(P.member(t, 25), 51, x=7.0, y=Y))
    # distance 50 = TH_LOW is taken (bestDist starts at TH_LOW, `dist > TH_LOW` skips), 51 is not
    for node, k in ((60, 50), (61, 51)):
        t, r = P.base_row()
        a = A.add(r, node, x=5.0, y=Y)
        b = Bs.add(P.member(t, k), node, x=6.0, y=Y)
        if k == 50:
            both(a, b)
    # nodes on one side only (front, middle, back) holding equal descriptors
    for na, nb in ((1, 2), (25, 26), (90, BACK_NODE)):
        t, r = P.base_row()
        A.add(r, na, x=5.0, y=Y)
        Bs.add(P.member(t, 0), nb, x=6.0, y=Y)
    for _ in range(pad):
        A.add(P.filler(), 70, x=5.0, y=Y)
        Bs.add(P.filler(), 71, x=6.0, y=Y)
    d = P.array()
    # KannalaBrandt8 key frames have no mvuRight (bStereo1 = bStereo2 = false): with bCoarse the outcome is "coarse", except that all of
    # nodes 40-44 take the epipole test and are dropped
    kb8 = {a: b for a, b in coarse.items() if a not in no_u_right}
    return A.finish(d, P.rng), Bs.finish(d, P.rng), dict(plain=plain, coarse=coarse, only_stereo=stereo, f0={}, f0_coarse=coarse, kb8_coarse=kb8)


def tri_pairs(f12_zero):
    """TRI_PAIR_DTYPE records, one per batch entry; f12_zero[b]: the degenerate pair"""
    p = np.zeros(len(f12_zero), TRI_PAIR_DTYPE)
    p["F12"] = TRI_F12
    p["F12"][np.array(f12_zero, bool)] = 0
    p["ep"] = TRI_EP
    p["level_sigma2_2"][:, :8] = TRI_SIGMA2
    p["scale_factors_2"][:, :8] = TRI_SCALE
    return p


def tri_kb8_pairs(B):
    """TRI_KB8_PAIR_DTYPE records of one fisheye camera per key frame (n_cams = 1); with bCoarse the poses and intrinsics are not read"""
    p = np.zeros(B, TRI_KB8_PAIR_DTYPE)
    p["n_cams"] = 1
    p["k1"][:, 0] = p["k2"][:, 0] = np.float32([190.0, 190.0, 255.0, 255.0, 0.003, 0.0007, -0.002, 0.0002])
    p["R12"][:, 0] = np.eye(3, dtype=np.float32).reshape(9)
    p["t12"][:, 0] = np.float32([0.1, 0.0, 0.0])
    p["ep"] = TRI_EP
    p["level_sigma2_1"][:, :8] = p["level_sigma2_2"][:, :8] = TRI_SIGMA2
    p["scale_factors_2"][:, :8] = TRI_SCALE
    return p


# ---- Fuse / SearchBySim3 --------------------------------------------------------------------------------------------------------------
# 640 x 480 image, 64 x 48 grid: cells of 10 px, cell = round(x / 10).  Key points sit at integer positions whose last digit is 0-3 or 6-9,
# away from the rounding boundary.
FUSE_GRID = (0.0, 0.0, float(np.float32(64) / np.float32(640)), float(np.float32(48) / np.float32(480)))
FUSE_R = 8.0


def _query(u, v, level=0, r=FUSE_R, ur=0.0, flags=Q_VALID):
    q = np.zeros((), QUERY_DTYPE)
    q["u"], q["v"], q["radius"], q["u_right"], q["min_level"], q["max_level"], q["flags"] = u, v, r, ur, level - 1, level, flags
    return q


class Frame:
    """key points given in ENUMERATION order of the windows that hold them; finish() numbers them so that index order differs from it"""

    def __init__(self):
        self.k = []

    def add(self, row, x, y, octave=0, ur=-1.0):
        self.k.append(dict(row=row, x=x, y=y, octave=octave, ur=ur))
        return len(self.k) - 1

    def finish(self, desc, pad_rows=()):
        """index order: clusters of one grid cell keep their order (insertion order inside a cell IS index order, Frame.cc:444-478), the
        cells are numbered from the last to the first, so a later cell of a window holds lower indices than an earlier one"""
        cell = [(round(k["x"] / 10), round(k["y"] / 10)) for k in self.k]
        cells = sorted(set(cell), reverse=True)
        order = [lab for c in cells for lab in range(len(self.k)) if cell[lab] == c]
        index = np.zeros(len(self.k), np.int64)
        index[order] = np.arange(len(order))
        n = len(self.k) + len(pad_rows)
        o = dict(kps=np.zeros(n, KP_DTYPE), desc=np.zeros((n, 32), np.uint8), u_right=np.full(n, -1, np.float32), index=index, n=n)
        for k, i in zip(self.k, index):
            o["kps"][i], o["desc"][i], o["u_right"][i] = keypoint(k["x"], k["y"], k["octave"]), desc[k["row"]], k["ur"]
        for j, r in enumerate(pad_rows):      # unrelated key points in a far corner: they fill an entry up to its capacity
            o["kps"][len(self.k) + j], o["desc"][len(self.k) + j] = keypoint(600.0 + j % 4, 400.0 + (j // 4) % 4), desc[r]
        return o


def _site(F, P, x0, y0, total, planted):
    """a cluster site of `total` key points around (x0 + 1, y0 + 1), spread over the cells (cx, cy), (cx, cy + 1), (cx + 1, cy) of a window
    of radius 8 there in enumeration order (ix outer, iy inner, index order inside a cell).  planted: {enumeration position: row}; unrelated
    rows elsewhere.  -> labels by enumeration position"""
    sizes = [total - 2 * (total // 3), total // 3, total // 3]
    at = [(x0, y0), (x0, y0 + 6), (x0 + 6, y0)]
    labs = []
    for (cx, cy), m in zip(at, sizes):
        for j in range(m):
            p = len(labs)
            labs.append(F.add(planted[p] if p in planted else P.filler(), cx + j % 3, cy + (j // 3) % 3))
    return labs


def fuse_case(seed, pad=0):
    """Fuse without the chi2 gate (the Sim3 overload, :1884-2006) at th_dist = TH_LOW = 50.
    -> (frame, queries QUERY_DTYPE [nq], qdesc, expected [(key point label or -1, bestDist)] per query)"""
    P = Pool(seed)
    F = Frame()
    Q, QD, exp = [], [], []

    def ask(q, row, lab, dist):
        Q.append(q); QD.append(row); exp.append((lab, dist))

    sites = {}
    # three sites whose window (u, v) = (x0 + 1, y0 + 1), r = 8 holds 65, 128 and 200 entries; per site the queries' tracks are planted first
    plan = {65: (100, 100), 128: (300, 100), 200: (500, 100)}
    tracks = {n: [P.base_row() for _ in range(3)] for n in plan}
    for n, (x0, y0) in plan.items():
        t0, t1, t2 = [t for t, _ in tracks[n]]
        planted = {}
        if n == 65:
            planted = {63: P.member(t0, 10), 64: P.member(t0, 10),      # equal distances across the chunk boundary: the first (63) wins
                       2: P.member(t1, 30), 64 - 4: P.member(t1, 9)}    # best late in the first chunk
        if n == 128:
            planted = {60: P.member(t0, 10), 100: P.member(t0, 10),     # equal distances in chunks 1 and 2: position 60 wins
                       70: P.member(t1, 10), 5: P.member(t1, 11),       # best in the second chunk, a near miss in the first
                       127: P.member(t2, 50)}                           # dist == th_dist at the very last entry: accepted
        if n == 200:
            planted = {150: P.member(t0, 10), 20: P.member(t0, 11), 90: P.member(t0, 12),     # best in the third chunk
                       64: P.member(t1, 7), 128: P.member(t1, 7), 192: P.member(t1, 7),       # equal at the start of chunks 2, 3, 4: 64 wins
                       199: P.member(t2, 51)}                                                 # 51 > th_dist: refused, q_dist = 51
        sites[n] = _site(F, P, x0, y0, n, planted)
    for n, (x0, y0) in plan.items():
        rows = [r for _, r in tracks[n]]
        L = sites[n]
        if n == 65:
            ask(_query(x0 + 1, y0 + 1), rows[0], L[63], 10); ask(_query(x0 + 1, y0 + 1), rows[1], L[60], 9)
        if n == 128:
            ask(_query(x0 + 1, y0 + 1), rows[0], L[60], 10); ask(_query(x0 + 1, y0 + 1), rows[1], L[70], 10); ask(_query(x0 + 1, y0 + 1), rows[2], L[127], 50)
        if n == 200:
            ask(_query(x0 + 1, y0 + 1), rows[0], L[150], 10); ask(_query(x0 + 1, y0 + 1), rows[1], L[64], 7); ask(_query(x0 + 1, y0 + 1), rows[2], -1, 51)
    # |dx| == r exactly (strict `<`, KeyFrame.cc GetFeaturesInArea): the key point at x = u + 8 is outside, the one at 60 (> 50) is the best
    t, r = P.base_row()
    F.add(P.member(t, 0), 209.0, 301.0); F.add(P.member(t, 60), 203.0, 301.0)
    ask(_query(201.0, 301.0), r, -1, 60)
    t, r = P.base_row()                                            # same with |dy| == r, and an accepted neighbour at |dy| = 7
    F.add(P.member(t, 0), 301.0, 309.0); near = F.add(P.member(t, 40), 301.0, 308.0)
    ask(_query(301.0, 301.0), r, near, 40)
    # level filter (:1790 / :2193): nPredictedLevel = 2 takes levels 1 and 2; the nearer candidates at levels 0 and 3 are skipped
    t, r = P.base_row()
    F.add(P.member(t, 3), 400.0, 300.0, octave=0); F.add(P.member(t, 4), 401.0, 300.0, octave=3)
    l1 = F.add(P.member(t, 20), 402.0, 300.0, octave=1); F.add(P.member(t, 21), 403.0, 300.0, octave=2)
    ask(_query(401.0, 301.0, level=2), r, l1, 20)
    # windows clamped at the four image borders, each with its key point, and windows wholly outside (no cell: bestDist stays 256)
    for (u, v), (x, y) in (((2.0, 240.0), (3.0, 241.0)), ((637.0, 240.0), (633.0, 241.0)), ((320.0, 2.0), (321.0, 3.0)), ((320.0, 477.0), (321.0, 473.0))):
        t, r = P.base_row()
        ask(_query(u, v), r, F.add(P.member(t, 25), x, y), 25)
    for u, v in ((-50.0, 240.0), (700.0, 240.0), (320.0, -50.0), (320.0, 540.0)):
        ask(_query(u, v), P.filler(), -1, 256)
    # Q_VALID cleared on a query with a perfect candidate: no search (q_dist = 256)
    t, r = P.base_row()
    F.add(P.member(t, 0), 100.0, 400.0)
    ask(_query(101.0, 401.0, flags=0), r, -1, 256)
    pad_rows = [P.filler() for _ in range(pad)]
    d = P.array()
    fr = F.finish(d, pad_rows)
    return fr, np.array(Q, QUERY_DTYPE), d[np.array(QD)], exp


def fuse_chi2_case(seed):
    """Fuse with the reprojection gate (:1793-1817), invLevelSigma2 = 1 / 1.44^level.  The query sits at (101, 101) with ur = 50.
    -> (frame, queries, qdesc, expected, inv_level_sigma2)"""
    P = Pool(seed)
    F = Frame()
    Q, QD, exp = [], [], []
    inv = (np.float32(1) / TRI_SIGMA2).astype(np.float32)
    cases = [
        # (candidates (dx, dy, u_right, octave, distance), expected candidate or -1, bestDist)
        ([(2, 1, -1.0, 0, 5), (1, 1, -1.0, 0, 30)], 0, 5),       # monocular e2 = 5 <= 5.99: the nearer one passes
        ([(2, 2, -1.0, 0, 5), (1, 1, -1.0, 0, 30)], 1, 30),      # e2 = 8 > 5.99: skipped
        ([(2, 1, 49.0, 0, 5), (1, 1, -1.0, 0, 30)], 0, 5),       # stereo, er = 1: e2 = 6 <= 7.8
        ([(2, 1, 48.0, 0, 5), (1, 1, -1.0, 0, 30)], 1, 30),      # stereo, er = 2: e2 = 9 > 7.8 (monocular it would pass with 5)
        ([(2, 2, 50.0, 0, 5), (1, 1, -1.0, 0, 30)], 1, 30),      # stereo, er = 0: e2 = 8 > 7.8
        ([(2, 2, -1.0, 1, 5), (1, 1, -1.0, 0, 30)], 0, 5),       # level 1: 8 / 1.44 = 5.56 <= 5.99
    ]
    for j, (cands, want, dist) in enumerate(cases):
        x0, y0 = 100.0 + 60 * j, 100.0
        t, r = P.base_row()
        labs = [F.add(P.member(t, k), x0 + 1 + dx, y0 + 1 + dy, octave=o, ur=ur) for dx, dy, ur, o, k in cands]
        Q.append(_query(x0 + 1, y0 + 1, level=1, ur=50.0)); QD.append(r); exp.append((labs[want], dist))
    # mvuRight = 0.0 is a stereo key point (`>= 0`, :1793): er = 50 - 0 -> e2 = 2505: skipped, where a monocular one at the same place passes
    t, r = P.base_row()
    F.add(P.member(t, 5), 102.0, 301.0, ur=0.0); m = F.add(P.member(t, 30), 100.0, 301.0)
    Q.append(_query(101.0, 301.0, level=1, ur=50.0)); QD.append(r); exp.append((m, 30))
    d = P.array()
    return F.finish(d), np.array(Q, QUERY_DTYPE), d[np.array(QD)], exp, inv


def sim3_case(seed, pad=0):
    """SearchBySim3 (:2008-2220): one query slot per key point in both directions (th_dist = TH_HIGH); isolated pairs of key points 40 px apart.
    -> (frame 1, frame 2, q12, q12desc, q21, q21desc, expected {label in 1: label in 2})"""
    P = Pool(seed)
    F1, F2 = Frame(), Frame()
    exp = {}
    spec = []   # (label in 1, label in 2, query of 1 into 2 valid, query of 2 into 1 valid)
    # per site (valid 1 -> 2, valid 2 -> 1, distance, matched): mutual; 1 -> 2 only; 2 -> 1 only; neither; distance 100 = TH_HIGH; 101 refused
    kinds = [(1, 1, 10, True), (1, 0, 10, False), (0, 1, 10, False), (0, 0, 10, False), (1, 1, 100, True), (1, 1, 101, False)]
    for j, (v12, v21, k, ok) in enumerate(kinds):
        x, y = 40.0 + 40 * (j % 12), 40.0 + 40 * (j // 12)
        t, r = P.base_row()
        a = F1.add(r, x, y); b = F2.add(P.member(t, k), x + 1, y + 1)
        spec.append((a, b, v12, v21))
        if ok:
            exp[a] = b
    # a one-directional pair with every query valid: a (the base) and a2 (14 bits off) sit in one window of frame 1, b (10 bits off) in frame 2
    t, r = P.base_row()
    a = F1.add(r, 300.0, 300.0); a2 = F1.add(P.member(t, 14), 302.0, 300.0)
    b = F2.add(P.member(t, 10), 301.0, 301.0)
    # a -> b (10) and a2 -> b (24), but b -> a (10 against 24): a and b agree, a2's match is one-directional
    spec += [(a, b, 1, 1), (a2, None, 1, 0)]
    exp[a] = b
    d_rows1 = [P.filler() for _ in range(pad)]
    d_rows2 = [P.filler() for _ in range(pad)]
    d = P.array()
    f1, f2 = F1.finish(d, d_rows1), F2.finish(d, d_rows2)
    q12 = np.zeros(f1["n"], QUERY_DTYPE); q21 = np.zeros(f2["n"], QUERY_DTYPE)
    for a, b, v12, v21 in spec:
        ka = f1["kps"][f1["index"][a]]
        q12[f1["index"][a]] = _query(ka["x"], ka["y"], flags=Q_VALID if v12 else 0)
        if b is not None:
            kb = f2["kps"][f2["index"][b]]
            q21[f2["index"][b]] = _query(kb["x"], kb["y"], flags=Q_VALID if v21 else 0)
    return f1, f2, q12, f1["desc"].copy(), q21, f2["desc"].copy(), exp


def mutual_case():
    """orbm_mutual_matches (:2203-2219) on hand-written lists: cap1 = 300 with n1 = 257 (a second workgroup with one live thread), cap2 = 40
    with n2 = 30.  The slack of m21 behind n2 is a trap: m21[n2 + j] names the i1 whose m12 points there.
    -> (m12 [300], m21 [40], n1, n2, expected [300], count)"""
    cap1, cap2, n1, n2 = 300, 40, 257, 30
    m12 = np.full(cap1, -1, np.int32); m21 = np.full(cap2, -1, np.int32)
    exp = np.full(cap1, -1, np.int32)
    for i1, i2 in ((0, 5), (63, 0), (64, 29), (255, 7), (256, 8)):      # agreeing pairs, at wave and workgroup boundaries
        m12[i1], m21[i2], exp[i1] = i2, i1, i2
    m12[10], m21[11] = 11, 12                                           # one-directional: 10 -> 11 but 11 -> 12
    m12[12] = 3                                                         # 12 -> 3 but 3 -> nothing
    m21[20] = 40                                                        # 20 -> 40 but 40 -> nothing
    m12[100], m21[30] = 30, 100                                         # m12 entry == n2: behind the count, although the slack agrees
    m12[101], m21[39] = 39, 101                                         # m12 entry > n2
    m12[257], m21[9] = 9, 257                                           # i1 == n1: behind the count, although both lists agree
    m12[299], m21[10] = 10, 299
    return m12, m21, n1, n2, exp, 5


# ---- SearchForInitialization ----------------------------------------------------------------------------------------------------------
def init_case(seed, pad=0):
    """windowSize = 20, mfNNratio = 0.9, orientation check on (factor HISTO_LENGTH / 360, :851: bin = round(rot / 12)).  F1 features are
    visited in index order, so the labels ARE the indices here (no renumbering).
    -> dict(k1, d1, k2, d2, prev0, and per call the expected vnMatches12, nmatches, vbPrevMatched)"""
    P = Pool(seed)
    k1, r1, prev, k2, r2 = [], [], [], [], []

    def f1(row, px, py, octave=0, angle=0.0):
        k1.append(keypoint(px, py, octave, angle)); r1.append(row); prev.append((px, py))
        return len(k1) - 1

    def f2(row, x, y, octave=0, angle=0.0):
        k2.append(keypoint(x, y, octave, angle)); r2.append(row)
        return len(k2) - 1

    m1, m2 = {}, {}      # expected matches of the first and the second call
    # the steal chain on X: A (20) takes it, B (10) takes it from A (vnMatches12[A] = -1, nmatches--), C arrives at exactly 10 and is
    # refused by `vMatchedDistance[i2] <= dist` (:899).  A's rotation difference is 96 -> bin 8, B's is 0 -> bin 0
    t, r = P.base_row()
    X = f2(r, 100.0, 100.0)
    A = f1(P.member(t, 20), 101.0, 100.0, angle=96.0); B = f1(P.member(t, 10), 100.0, 101.0); C = f1(P.member(t, 10), 99.0, 100.0)
    m1[B] = X
    # level1 > 0 is ignored (:865) although its candidate is perfect; an F2 key point above level 0 is not a candidate (level1, level1)
    t, r = P.base_row()
    f1(r, 200.0, 100.0, octave=1); f2(P.member(t, 0), 200.0, 100.0)
    t, r = P.base_row()
    f1(r, 260.0, 100.0); f2(P.member(t, 0), 260.0, 100.0, octave=1)
    # ratio: bestDist < (float)bestDist2 * 0.9f (:915): 20 * 0.9f = 18.0f exactly after rounding: 18 fails, 17 passes
    for x, k in ((300.0, 18), (360.0, 17)):
        t, r = P.base_row()
        a = f1(r, x, 100.0)
        b = f2(P.member(t, k), x + 1, 100.0); f2(P.member(t, 20), x + 2, 100.0)
        if k == 17:
            m1[a] = b
    # three more matches in bin 0, one each in bins 3 and 5 (rot 36, 60), one in bin 10 (rot 120)
    for j, ang in enumerate((0.0, 0.0, 0.0, 36.0, 60.0, 120.0)):
        t, r = P.base_row()
        a = f1(r, 100.0 + 50 * j, 200.0, angle=ang)
        b = f2(P.member(t, 10), 101.0 + 50 * j, 200.0)
        if ang != 120.0:
            m1[a] = b
    # histogram: bin 0 = {B, 17-pair, three more, H} = 6, bin 3 = 1, bin 5 = 1, bin 8 = {A, stale} = 1, bin 10 = 1.  Strictly-larger updates keep
    # bins 0, 3, 5; bins 8 and 10 are culled: the bin-10 match goes (nmatches--), A's stale entry has vnMatches12 = -1 already and must
    # not be counted again (:963).
    # H: its window holds Z1 (20) only; Z2 (5) is 24 px from vbPrevMatched[H] but 12 px from Z1.  The first call matches Z1 and moves
    # vbPrevMatched[H] there (:976); the second call then sees both: 5 < 20 * 0.9 -> Z2
    t, r = P.base_row()
    H = f1(r, 400.0, 300.0)
    Z1 = f2(P.member(t, 20), 412.0, 300.0); Z2 = f2(P.member(t, 5), 424.0, 300.0)
    m1[H] = Z1
    for j in range(pad):
        f1(P.filler(), 30.0 + 4 * j, 400.0); f2(P.filler(), 30.0 + 4 * j, 440.0)
    m2 = dict(m1); m2[H] = Z2
    d = P.array()
    k1a, k2a = np.array(k1, KP_DTYPE), np.array(k2, KP_DTYPE)
    out = dict(k1=k1a, d1=d[np.array(r1)], k2=k2a, d2=d[np.array(r2)], prev0=np.array(prev, np.float32), calls=[])
    pv = out["prev0"]
    for m in (m1, m2):
        e = np.full(len(k1), -1, np.int32)
        pv = pv.copy()
        for a, b in m.items():
            e[a] = b
            pv[a] = (k2a["x"][b], k2a["y"][b])
        out["calls"].append(dict(match=e, n=len(m), prev=pv))
    return out
