"""Place recognition on the device (bowdb_detect_relocalization_candidates / bowdb_detect_n_best_candidates) against a literal Python
restatement of KeyFrameDatabase::DetectRelocalizationCandidates (KeyFrameDatabase.cc:785-897), KeyFrameDatabase::DetectNBestCandidates
(:614-782) and L1Scoring::score (DBoW2 ScoringObject.cpp:23-68).

The restatement keeps what the reference keeps: one list of key frames per word, filled by add in call order and edited by erase, and per key
frame the mnRelocQuery / mnRelocWords / mRelocScore and mnPlaceRecognitionQuery / ...Words / ...Score members with the reference's `!=` tests.
Scores are summed in Python floats (doubles) term by term and narrowed with np.float32; std::list::sort(compFirst) is a sort on
(-acc, position), i.e. explicitly stable.  Every comparison is exact: candidate lists, counts, stats and the score / last_query state of every
slot after every call (bit patterns).  backend "emu": the product kernels compiled against tests/emu; "hip": the real library on an MI355X."""
import bisect

import numpy as np
import pytest

import oracle_lib as O
from devarrays import BACKENDS, lib  # noqa: F401
from orbhip._lib import ORB_E_CAPACITY, ORB_E_INVALID, OrbHipError
from orbhip.bow import ORBVocabulary, synth_vocabulary
from orbhip.keyframe_db import KeyFrameDatabase, QueryBows, View, stats_of, to_host

f32 = np.float32


def device_of(backend):
    return None if backend == "emu" else "cuda:0"


# ------------------------------------------------------------------------------------------------ restatement of the reference
def l1_score(w1, v1, w2, v2):
    """L1Scoring::score (ScoringObject.cpp:23-68) on two BowVectors given as ascending word lists and value lists"""
    i, j, n1, n2 = 0, 0, len(w1), len(w2)
    score = 0.0
    while i < n1 and j < n2:
        vi, wi = v1[i], v2[j]
        if w1[i] == w2[j]:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif w1[i] < w2[j]:
            i = bisect.bisect_left(w1, w2[j], i)    # v1.lower_bound(v2_it->first)
        else:
            j = bisect.bisect_left(w2, w1[i], j)
    return -score / 2.0


class RefKF:
    def __init__(self, slot, words, values, map_id):
        self.slot, self.words, self.values, self.map = slot, [int(w) for w in words], [float(v) for v in values], map_id
        self.covis = []          # GetBestCovisibilityKeyFrames(10)
        self.mnRelocQuery = self.mnRelocWords = self.mnPlaceRecognitionQuery = self.mnPlaceRecognitionWords = 0
        self.mRelocScore = self.mPlaceRecognitionScore = f32(0)
        self.left_by = {"reloc": None, "place": None}    # id of the query that stored the score (test bookkeeping)


class RefDB:
    """mvInvertedFile + the two Detect functions; `log` receives one dict of counters per query"""

    def __init__(self):
        self.inv = {}
        self.log = []
        self.map_bad = set()

    def add(self, kf):
        for w in kf.words:
            self.inv.setdefault(w, []).append(kf)

    def erase(self, kf):
        for w in kf.words:
            if kf in self.inv.get(w, []):
                self.inv[w].remove(kf)

    def clear(self):
        self.inv = {}

    def clear_map(self, m):
        for w in self.inv:
            self.inv[w] = [k for k in self.inv[w] if k.map != m]

    def _accumulate(self, lScoreAndMatch, qid, fam, scored, entry):
        lAcc, bestAccScore = [], f32(0)
        Q, S = ("mnRelocQuery", "mRelocScore") if fam == "reloc" else ("mnPlaceRecognitionQuery", "mPlaceRecognitionScore")
        for si, kfi in lScoreAndMatch:
            bestScore = accScore = si
            best = kfi
            for kf2 in kfi.covis:
                if getattr(kf2, Q) != qid:
                    continue
                s2 = getattr(kf2, S)
                if kf2 not in scored and kf2.left_by[fam] is not None:
                    entry["stale_reads"] += 1
                accScore = f32(accScore + s2)
                if s2 > bestScore:
                    best, bestScore = kf2, s2
            lAcc.append((accScore, best))
            if accScore > bestAccScore:
                bestAccScore = accScore
        entry["best_acc"] = bestAccScore
        entry["accs"] = [a for a, _ in lAcc]
        return lAcc, bestAccScore

    def DetectRelocalizationCandidates(self, fid, words, values, pMap):
        entry = dict(n_sharing=0, max_common=0, n_scored=0, best_acc=f32(0), stale_reads=0, accs=[], pairs=[])
        self.log.append(entry)
        lKFsSharingWords = []
        for w in words:
            for kfi in self.inv.get(w, []):
                if kfi.mnRelocQuery != fid:
                    kfi.mnRelocWords = 0
                    kfi.mnRelocQuery = fid
                    lKFsSharingWords.append(kfi)
                kfi.mnRelocWords += 1
        if not lKFsSharingWords:
            return []
        maxCommonWords = max(k.mnRelocWords for k in lKFsSharingWords)
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        entry.update(n_sharing=len(lKFsSharingWords), max_common=maxCommonWords, min_common=minCommonWords,
                     words=[k.mnRelocWords for k in lKFsSharingWords])
        lScoreAndMatch = []
        for kfi in lKFsSharingWords:
            if kfi.mnRelocWords > minCommonWords:
                si = f32(l1_score(words, values, kfi.words, kfi.values))
                kfi.mRelocScore = si
                kfi.left_by["reloc"] = fid
                lScoreAndMatch.append((si, kfi))
                entry["pairs"].append(kfi.slot)
        entry["n_scored"] = len(lScoreAndMatch)
        if not lScoreAndMatch:
            return []
        lAcc, bestAccScore = self._accumulate(lScoreAndMatch, fid, "reloc", {k for _, k in lScoreAndMatch}, entry)
        minScoreToRetain = f32(0.75) * bestAccScore
        already, out = set(), []
        entry["dropped_other_map"] = entry["dups"] = entry["at_threshold"] = 0
        for si, kfi in lAcc:
            entry["at_threshold"] += int(si == minScoreToRetain)
            if si > minScoreToRetain:
                if kfi.map != pMap:
                    entry["dropped_other_map"] += 1
                    continue
                if kfi not in already:
                    out.append(kfi.slot)
                    already.add(kfi)
                else:
                    entry["dups"] += 1
        return out

    def DetectNBestCandidates(self, kid, words, values, pMap, connected, nNumCandidates):
        entry = dict(n_sharing=0, max_common=0, n_scored=0, best_acc=f32(0), stale_reads=0, accs=[], pairs=[], dups=0, connected_hit=0)
        self.log.append(entry)
        lKFsSharingWords = []
        for w in words:
            for kfi in self.inv.get(w, []):
                if kfi.mnPlaceRecognitionQuery != kid:
                    kfi.mnPlaceRecognitionWords = 0
                    if kfi not in connected:
                        kfi.mnPlaceRecognitionQuery = kid
                        lKFsSharingWords.append(kfi)
                    else:
                        entry["connected_hit"] += 1
                kfi.mnPlaceRecognitionWords += 1
        if not lKFsSharingWords:
            return [], []
        maxCommonWords = max(k.mnPlaceRecognitionWords for k in lKFsSharingWords)
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        entry.update(n_sharing=len(lKFsSharingWords), max_common=maxCommonWords, min_common=minCommonWords,
                     words=[k.mnPlaceRecognitionWords for k in lKFsSharingWords])
        lScoreAndMatch = []
        for kfi in lKFsSharingWords:
            if kfi.mnPlaceRecognitionWords > minCommonWords:
                si = f32(l1_score(words, values, kfi.words, kfi.values))
                kfi.mPlaceRecognitionScore = si
                kfi.left_by["place"] = kid
                lScoreAndMatch.append((si, kfi))
                entry["pairs"].append(kfi.slot)
        entry["n_scored"] = len(lScoreAndMatch)
        if not lScoreAndMatch:
            return [], []
        lAcc, _ = self._accumulate(lScoreAndMatch, kid, "place", {k for _, k in lScoreAndMatch}, entry)
        lAcc = [p for _, p in sorted(enumerate(lAcc), key=lambda t: (-float(t[1][0]), t[0]))]    # lAccScoreAndMatch.sort(compFirst), stable
        loop, merge, already = [], [], set()
        i = 0
        while i < len(lAcc) and (len(loop) < nNumCandidates or len(merge) < nNumCandidates):
            kfi = lAcc[i][1]
            if kfi not in already:
                if pMap == kfi.map and len(loop) < nNumCandidates:
                    loop.append(kfi.slot)
                elif pMap != kfi.map and len(merge) < nNumCandidates and kfi.map not in self.map_bad:
                    merge.append(kfi.slot)
                already.add(kfi)
            else:
                entry["dups"] += 1
            i += 1
        return loop, merge


# ------------------------------------------------------------------------------------------------ the pair: restatement + device database
def normalised(vals):
    """BowVector::normalize(L1) (BowVector.cpp:60-84): the sum of |v| in order, then one division each"""
    norm = 0.0
    for v in vals:
        norm += abs(float(v))
    return [float(v) / norm for v in vals] if norm > 0 else [float(v) for v in vals]


class Pair:
    """the same database twice: RefDB / RefKF objects and a KeyFrameDatabase on `backend`; every query is run on both and compared"""

    def __init__(self, lib, backend, n_slots, cap_f, n_maps=4, cap_q=None, n_rows=64):
        self.backend, self.ref = backend, RefDB()
        self.db = KeyFrameDatabase(n_slots, cap_f, n_maps, device_of(backend), lib=lib)
        self.kfs = [None] * n_slots          # RefKF of the slot (kept after erase, as the reference keeps the KeyFrame)
        self.h_word, self.h_val, self.h_n = np.zeros((n_slots, cap_f), np.int32), np.zeros((n_slots, cap_f)), np.zeros(n_slots, np.int32)
        self.cap_q = cap_q or cap_f
        self.qs = dict(bv_word=self.db._zeros((n_rows, self.cap_q), np.int32), bv_value=self.db._zeros((n_rows, self.cap_q), np.float64),
                       bv_n=self.db._zeros((n_rows,), np.int32))
        self.n_rows = n_rows

    def put(self, dst, src):
        if self.backend == "emu":
            dst[...] = src
        else:
            import torch
            dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))

    def set_rows(self, slots, bows):
        """writes BowVector rows (the data movement of add) on both sides; bows[i] = (words, values)"""
        for s, (w, v) in zip(slots, bows):
            self.h_word[s] = 0; self.h_val[s] = 0
            self.h_word[s, :len(w)] = w; self.h_val[s, :len(w)] = v; self.h_n[s] = len(w)
        self.put(self.db.bv_word, self.h_word); self.put(self.db.bv_value, self.h_val); self.put(self.db.bv_n, self.h_n)

    def add(self, slots, maps):
        maps = np.broadcast_to(np.asarray(maps), (len(slots),))
        for s, m in zip(slots, maps):
            n = self.h_n[s]
            kf = RefKF(s, self.h_word[s, :n], self.h_val[s, :n], int(m))
            if self.kfs[s] is not None:
                kf.covis = self.kfs[s].covis
                for other in self.kfs:          # neighbours point at the new object
                    if other is not None:
                        other.covis = [kf if c is self.kfs[s] else c for c in other.covis]
            self.kfs[s] = kf
            self.ref.add(kf)
        self.db.add(slots, maps)

    def erase(self, slots):
        for s in slots:
            self.ref.erase(self.kfs[s])
        self.db.erase(slots)

    def set_covisibles(self, slots, lists):
        for s, l in zip(slots, lists):
            self.kfs[s].covis = [self.kfs[c] for c in l if 0 <= c < len(self.kfs) and self.kfs[c] is not None]
        self.db.set_covisibles(slots, lists)

    def expected_state(self, fam):
        q, s = np.zeros(len(self.kfs), np.uint64), np.zeros(len(self.kfs), f32)
        for i, k in enumerate(self.kfs):
            if k is not None:
                q[i] = k.mnRelocQuery if fam == "reloc" else k.mnPlaceRecognitionQuery
                s[i] = k.mRelocScore if fam == "reloc" else k.mPlaceRecognitionScore
        return q, s

    def check_state(self, fam):
        q, s = self.expected_state(fam)
        gq = to_host(self.db.reloc_query if fam == "reloc" else self.db.place_query).view(np.uint64)
        gs = to_host(self.db.reloc_score if fam == "reloc" else self.db.place_score)
        assert np.array_equal(gq, q), ("last_query", fam, np.nonzero(gq != q)[0][:8])
        assert np.array_equal(gs.view(np.uint32), s.view(np.uint32)), ("score", fam, np.nonzero(gs.view(np.uint32) != s.view(np.uint32))[0][:8])

    def load_queries(self, bows):
        w, v, n = np.zeros((self.n_rows, self.cap_q), np.int32), np.zeros((self.n_rows, self.cap_q)), np.zeros(self.n_rows, np.int32)
        for r, (ww, vv) in enumerate(bows):
            w[r, :len(ww)] = ww; v[r, :len(ww)] = vv; n[r] = len(ww)
        self.put(self.qs["bv_word"], w); self.put(self.qs["bv_value"], v); self.put(self.qs["bv_n"], n)

    def check_stats(self, res, log):
        st = stats_of(res)
        for k, e in enumerate(log):
            assert (st[k]["n_sharing"], st[k]["max_common_words"], st[k]["n_scored"]) == (e["n_sharing"], e["max_common"], e["n_scored"]), (k, st[k], e)
            assert st[k]["best_acc_score"].view(np.uint32) == f32(e["best_acc"]).view(np.uint32), (k, st[k], e["best_acc"])

    def reloc(self, ids, bows, maps, cap_cand=64, q_bows=None, rows=None):
        """one device call for all queries vs the restatement run query by query -> (candidate lists, log entries)"""
        n = len(ids)
        if q_bows is None:
            self.load_queries(bows)
            q_bows = self.qs
        Q = self.db.set_queries(self.db.make_queries("reloc", n), ids, maps, rows)
        res = self.db.DetectRelocalizationCandidates(Q, q_bows, cap_cand)
        maps = np.broadcast_to(np.asarray(maps), (n,))
        first = len(self.ref.log)
        want = [self.ref.DetectRelocalizationCandidates(ids[k], [int(x) for x in bows[k][0]], [float(x) for x in bows[k][1]], int(maps[k])) for k in range(n)]
        cand, nc, nr = to_host(res["cand"]), to_host(res["n_cand"]), to_host(res["n_required"])
        for k in range(n):
            assert nr[k] == len(want[k]) and nc[k] == min(len(want[k]), cap_cand), (k, nr[k], nc[k], want[k])
            assert list(cand[k, :nc[k]]) == want[k][:cap_cand], (k, list(cand[k, :nc[k]]), want[k])
        self.check_stats(res, self.ref.log[first:])
        self.check_state("reloc")
        return want, self.ref.log[first:], res

    def nbest(self, ids, bows, maps, conn, ncand=3, q_bows=None, rows=None):
        n = len(ids)
        if q_bows is None:
            self.load_queries(bows)
            q_bows = self.qs
        Q = self.db.set_queries(self.db.make_queries("place", n, cap_conn=sum(len(c) for c in conn)), ids, maps, rows, conn)
        res = self.db.DetectNBestCandidates(Q, q_bows, ncand)
        maps = np.broadcast_to(np.asarray(maps), (n,))
        first = len(self.ref.log)
        want = []
        for k in range(n):
            connected = {self.kfs[c] for c in conn[k] if 0 <= c < len(self.kfs) and self.kfs[c] is not None}
            want.append(self.ref.DetectNBestCandidates(ids[k], [int(x) for x in bows[k][0]], [float(x) for x in bows[k][1]], int(maps[k]), connected, ncand))
        lp, nl, mg, nm = (to_host(res[x]) for x in ("loop", "n_loop", "merge", "n_merge"))
        for k in range(n):
            wl, wm = want[k]
            assert (nl[k], nm[k]) == (len(wl), len(wm)), (k, nl[k], nm[k], want[k])
            assert list(lp[k, :nl[k]]) == wl and list(mg[k, :nm[k]]) == wm, (k, lp[k], mg[k], want[k])
            assert (lp[k, nl[k]:] == -1).all() and (mg[k, nm[k]:] == -1).all()
        self.check_stats(res, self.ref.log[first:])
        self.check_state("place")
        return want, self.ref.log[first:], res


# ------------------------------------------------------------------------------------------------ synthetic BowVectors
def zipf_words(rng, n_words, m, a=2.5):
    """m draws of a Zipf-like word id in [0, n_words) -> sorted distinct ids"""
    return np.unique((n_words * rng.random(m) ** a).astype(np.int64))


def bow_from_words(rng, words):
    return np.asarray(words, np.int32), normalised(rng.uniform(0.5, 9.0, len(words)))


def perturbed(rng, words, n_words, keep, m_new):
    """keeps each word with probability `keep` and draws m_new fresh ones"""
    w = np.asarray(words)
    kept = w[rng.random(len(w)) < keep]
    return np.unique(np.concatenate([kept, zipf_words(rng, n_words, m_new)]))


def random_world(rng, n_kf, n_words, m, cap_f):
    """key frames along a walk (each keeps most words of its predecessor, so neighbours in add order look alike), a few places revisited"""
    bows, cur = [], zipf_words(rng, n_words, m)
    for i in range(n_kf):
        if i and rng.random() < 0.03:
            cur = zipf_words(rng, n_words, m)                      # a jump to a new place
        elif i > 20 and rng.random() < 0.05:
            cur = np.asarray(bows[rng.integers(0, i)][0], np.int64)   # a revisit
        cur = perturbed(rng, cur, n_words, 0.85, max(m // 6, 1))[:cap_f]
        bows.append(bow_from_words(rng, cur))
    return bows


def covis_lists(rng, n_kf):
    """up to ten neighbours in add order (both directions), shuffled, sometimes fewer"""
    out = []
    for i in range(n_kf):
        near = [j for j in range(i - 8, i + 9) if j != i and 0 <= j < n_kf]
        rng.shuffle(near)
        out.append(near[:int(rng.integers(0, 11))])
    return out


def build_random_pair(lib, backend, seed, n_kf, n_words, m, n_maps=3, with_ref=True):
    rng = np.random.default_rng(seed)
    cap_f = min(4096, max(8, int(m * 1.3)))
    P = Pair(lib, backend, n_kf, cap_f, n_maps=n_maps)
    bows = random_world(rng, n_kf, n_words, m, cap_f)
    slots = list(range(n_kf))
    P.set_rows(slots, bows)
    P.add(slots, [min(i * n_maps // max(n_kf, 1), n_maps - 1) if rng.random() < 0.9 else int(rng.integers(0, n_maps)) for i in slots])
    P.set_covisibles(slots, covis_lists(rng, n_kf))
    return P, rng, bows


def query_sequence(rng, bows, n_words, nq, cap_q):
    """queries near existing key frames, clustered so that later queries revisit the neighbourhood of earlier ones (stale scores get read)"""
    out, anchor = [], int(rng.integers(0, len(bows)))
    for _ in range(nq):
        if rng.random() < 0.3:
            anchor = int(rng.integers(0, len(bows)))
        src = min(max(anchor + int(rng.integers(-3, 4)), 0), len(bows) - 1)
        out.append((src, bow_from_words(rng, perturbed(rng, bows[src][0], n_words, float(rng.uniform(0.6, 0.95)), max(len(bows[src][0]) // 8, 1))[:cap_q])))
    return out


def summarise(log):
    scored = sum(1 for e in log if e["n_scored"] >= 1)
    return scored, sum(e["stale_reads"] for e in log)


SIZES = [(1, 1000, 40), (50, 1000, 60), (2000, 100000, 100)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n_kf,n_words,m", SIZES)
def test_random_sequences_match_the_restatement(lib, backend, n_kf, n_words, m):
    """>= 20 queries per family against random databases, all queries of a family in ONE call; the same sequence again on a second copy of the
    database with one query per call: identical candidates, stats and state (both are compared with the restatement after every call)"""
    NQ = 20
    A, rng, bows = build_random_pair(lib, backend, 100 + n_kf, n_kf, n_words, m)
    B, _, _ = build_random_pair(lib, backend, 100 + n_kf, n_kf, n_words, m)
    qs = query_sequence(rng, bows, n_words, 2 * NQ, A.cap_q)
    ids = list(range(5, 5 + 3 * NQ, 3))
    qb = [b for _, b in qs]
    maps = [A.kfs[src].map if rng.random() < 0.8 else int(rng.integers(0, 3)) for src, _ in qs]
    conn = [[c for c in range(src - 2, src + 3) if 0 <= c < n_kf and n_kf > 1 and rng.random() < 0.7] + ([-1, n_kf + 5] if k % 5 == 0 else []) for k, (src, _) in enumerate(qs)]
    # one call
    wr, lr, _ = A.reloc(ids, qb[:NQ], maps[:NQ])
    wn, ln, _ = A.nbest(ids, qb[NQ:], maps[NQ:], conn[NQ:])
    for log in (lr, ln):
        scored, stale = summarise(log)
        assert scored >= 0.9 * NQ, scored
        if n_kf > 1:
            assert stale >= 1, "no covisible was accumulated with a score an earlier query left"
            assert max(e["max_common"] for e in log) >= 20 and any(e["n_scored"] < e["n_sharing"] for e in log)
    if n_kf > 1:
        assert any(len(w) >= 2 for w in wr) and any(len(l) + len(mg) >= 2 for l, mg in wn) and sum(e["connected_hit"] for e in ln) > 0
    # one query per call, on the second copy
    for k in range(NQ):
        w1, _, _ = B.reloc([ids[k]], [qb[k]], [maps[k]])
        assert w1[0] == wr[k]
    for k in range(NQ):
        w1, _, _ = B.nbest([ids[k]], [qb[NQ + k]], [maps[NQ + k]], [conn[NQ + k]])
        assert w1[0] == wn[k]
    for fam in ("reloc", "place"):
        qa, sa = A.expected_state(fam)
        qb_, sb = B.expected_state(fam)
        assert np.array_equal(qa, qb_) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32))


@pytest.mark.gpu
def test_random_sequence_20000_keyframes_hip(hip_lib):
    """20 000 key frames x ~1 000 words: the pair scores and every output against the restatement"""
    P, rng, bows = build_random_pair(hip_lib, "hip", 7, 20000, 1000000, 950)
    assert 800 < np.mean([len(b[0]) for b in bows]) < 1300
    NQ = 20
    qs = query_sequence(rng, bows, 1000000, 2 * NQ, P.cap_q)
    ids = list(range(1, NQ + 1))
    _, lr, _ = P.reloc(ids, [b for _, b in qs[:NQ]], [P.kfs[s].map for s, _ in qs[:NQ]])
    _, ln, _ = P.nbest(ids, [b for _, b in qs[NQ:]], [P.kfs[s].map for s, _ in qs[NQ:]], [[s] for s, _ in qs[NQ:]])
    for log in (lr, ln):
        scored, stale = summarise(log)
        assert scored >= 0.9 * NQ and stale >= 1, (scored, stale)
        assert max(e["max_common"] for e in log) >= 200


@pytest.mark.parametrize("backend", BACKENDS)
def test_pair_scores_match_the_oracle(lib, backend):
    """the restatement's pair score == the oracle's obw_score_l1 bit for bit, and the device stores its float narrowing"""
    P, rng, bows = build_random_pair(lib, backend, 3, 40, 2000, 80)
    qs = query_sequence(rng, bows, 2000, 6, P.cap_q)
    _, log, _ = P.reloc(list(range(1, 7)), [b for _, b in qs], 0)
    n = 0
    for e, (_, (w, v)) in zip(log, qs):
        for slot in e["pairs"]:
            k = P.kfs[slot]
            want = O.bow_score_l1(w, np.array(v), np.array(k.words, np.int32), np.array(k.values))
            got = l1_score([int(x) for x in w], v, k.words, k.values)
            assert np.float64(want).view(np.uint64) == np.float64(got).view(np.uint64)
            n += 1
    assert n >= 10


# ------------------------------------------------------------------------------------------------ hand-built cases
def simple_bow(words, vals=None):
    words = sorted(words)
    return np.asarray(words, np.int32), normalised(vals if vals is not None else [1.0 + 0.37 * (w % 7) for w in words])


def small_pair(lib, backend, bows, maps=0, n_slots=None, cap_f=32, covis=None, n_maps=4):
    n = len(bows)
    P = Pair(lib, backend, n_slots or n, cap_f, n_maps=n_maps)
    P.set_rows(range(n), bows)
    P.add(list(range(n)), maps)
    if covis:
        P.set_covisibles(list(range(n)), covis)
    return P


@pytest.mark.parametrize("backend", BACKENDS)
def test_ties_keep_list_order(lib, backend):
    """duplicated BowVectors give equal acc; N-best must keep the list order (first common word, then add order) among them"""
    dup = simple_bow([3, 5, 9, 12])
    other = simple_bow([1, 5, 9, 12, 20])
    bows = [dup, other, dup, dup, simple_bow([0, 3, 5, 9, 12]), dup]
    P = small_pair(lib, backend, bows, maps=[0, 0, 0, 1, 0, 1])
    P.erase([0]); P.set_rows([0], [dup]); P.add([0], [0])      # slot 0 moves to the back of the lists: its equal acc now comes last
    q = simple_bow([3, 5, 9, 12])
    (want,), (e,), _ = P.nbest([4], [q], 0, [[]], ncand=64)
    accs = [a.view(np.uint32) for a in e["accs"]]
    assert len(set(accs)) < len(accs), "no tie"
    # common words: 4 for the duplicates and slot 4, 3 for slot 1 (not scored: 3 > (int)(4 * 0.8f) fails).  The duplicates equal the query, so
    # they tie at the top; list order among them = add order with slot 0 last
    assert want == ([2, 0, 4], [3, 5]), want
    (wr,), _, _ = P.reloc([4], [q], 0)
    assert [s for s in wr if s != 4] == [2, 0], wr


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("M", [1, 4, 5, 6, 10])
def test_common_word_threshold_boundary(lib, backend, M):
    """key frames at exactly minCommonWords (not scored) and minCommonWords + 1 (scored)"""
    mn = int(f32(M) * f32(0.8))
    q = simple_bow(range(20))
    bows = [simple_bow(list(range(M)) + [100, 101]), simple_bow(list(range(mn)) + [200, 201, 202]), simple_bow(list(range(min(mn + 1, M))) + [300])]
    P = small_pair(lib, backend, bows)
    for fam_call in (lambda: P.reloc([9], [q], 0), lambda: P.nbest([9], [q], 0, [[]])):
        _, (e,), _ = fam_call()
        assert e["max_common"] == M and e["min_common"] == mn
        assert 0 in e["pairs"] and 2 in e["pairs"] and 1 not in e["pairs"]
        assert e["n_sharing"] == (3 if mn > 0 else 2)


@pytest.mark.parametrize("backend", BACKENDS)
def test_database_edits_and_degenerate_rows(lib, backend):
    """erase then re-add (new seq, moves to the back), clear_map, a query sharing nothing, bv_n = 0 and bv_n = cap_f rows, a query aliasing a row"""
    cap = 16
    full = simple_bow(range(10, 10 + cap))
    bows = [simple_bow([10, 11, 12, 13]), simple_bow([10, 11, 12, 14]), (np.zeros(0, np.int32), []), full, simple_bow([10, 11, 12, 15]), simple_bow([11, 12, 13])]
    P = small_pair(lib, backend, bows, maps=[0, 0, 0, 0, 1, 1], cap_f=cap, n_slots=8)      # slots 6, 7 never added
    q = simple_bow([10, 11, 12])
    (w0,), (e,), _ = P.reloc([1], [q], 0)
    assert w0[:2] == [0, 1] and e["n_sharing"] == 5
    P.erase([0]); P.set_rows([0], [bows[0]]); P.add([0], [0])
    (w1,), _, _ = P.reloc([2], [q], 0)
    assert w1[:2] == [1, 0], w1      # slot 0 now after every other key frame holding word 10
    (wn,), (e,), _ = P.reloc([3], [simple_bow([500, 501])], 0)
    assert wn == [] and (e["n_sharing"], e["max_common"], e["n_scored"]) == (0, 0, 0)
    # a query that is a database row (aliasing): row 3, bv_n == cap_f
    (wa,), (e,), _ = P.reloc([4], [full], 0, q_bows=P.db.rows(0, 8), rows=[3])
    assert wa == [3] and e["max_common"] == cap
    # an empty query row
    (we,), _, _ = P.reloc([5], [bows[2]], 0, q_bows=P.db.rows(0, 8), rows=[2])
    assert we == []
    P.ref.clear_map(1); P.db.clear_map(1)
    (w2,), (e,), _ = P.nbest([1], [q], 1, [[]])
    assert e["n_sharing"] == 3 and w2[0] == [] and sorted(w2[1]) == [0, 1, 3], w2
    P.ref.clear(); P.db.clear()
    (w3,), (e,), _ = P.nbest([2], [q], 0, [[]])
    assert w3 == ([], []) and e["n_sharing"] == 0
    (w4,), _, _ = P.reloc([6], [q], 0)
    assert w4 == []


@pytest.mark.parametrize("backend", BACKENDS)
def test_empty_database(lib, backend):
    P = Pair(lib, backend, 0, 8)
    assert P.reloc([1, 2], [simple_bow([1, 2])] * 2, 0)[0] == [[], []]
    assert P.nbest([1], [simple_bow([1, 2])], 0, [[]])[0] == [([], [])]


@pytest.mark.parametrize("backend", BACKENDS)
def test_n_best_walk(lib, backend):
    """connected key frames excluded with their state untouched; loop list full before the merge list and the reverse; a bad map; two entries
    electing the same bestKF; n_candidates 1, 3, 64; covisibility entries that are -1, not present, out of range"""
    q = simple_bow([1, 2, 3, 4, 5])
    # slot 10 equals the query (the best score); every other key frame has one private word more
    bows = [simple_bow([1, 2, 3, 4, 5] + [50 + i]) for i in range(10)] + [q] + [simple_bow([1, 2, 3, 4, 5] + [80 + i]) for i in range(2)]
    maps = [0, 0, 0, 0, 1, 1, 1, 2, 2, 0, 0, 0, 0]
    covis = [[10, -1, 99], [10], [], [], [4], [], [], [], [], [9, 3], [], [], []]      # 0 and 1 elect slot 10, as slot 10 itself does
    P = small_pair(lib, backend, bows, maps=maps, covis=covis, n_slots=15)
    P.set_rows([13], [simple_bow([1, 2, 3, 4, 5, 70])])                  # slot 13: a row that was never added (not present)
    P.db.set_covisibles([2], [[13, 99, 5]])
    P.kfs[2].covis = [P.kfs[5]]
    before = P.expected_state("place")
    (w3,), (e,), _ = P.nbest([10], [q], 0, [[9, 3]], ncand=3)
    assert e["connected_hit"] >= 2 and e["dups"] == 2 and 10 in w3[0], (e, w3)
    after = P.expected_state("place")
    assert after[0][9] == before[0][9] == 0 and after[0][3] == 0
    assert len(w3[0]) == 3 and len(w3[1]) == 3
    (w1,), _, _ = P.nbest([11], [q], 0, [[9, 3]], ncand=1)
    assert w1 == ([w3[0][0]], [w3[1][0]])
    P.ref.map_bad.add(1); P.db.set_map_bad(1)
    (w64,), _, _ = P.nbest([12], [q], 0, [[]], ncand=64)
    assert all(P.kfs[s].map == 2 for s in w64[1]) and len(w64[1]) == 2 and len(w64[0]) >= 4
    (wm,), _, _ = P.nbest([13], [q], 2, [[]], ncand=2)               # query in map 2: loop = map 2, merge = map 0 only (map 1 is bad)
    assert len(wm[0]) == 2 and len(wm[1]) == 2 and all(P.kfs[s].map == 0 for s in wm[1])
    P.ref.map_bad.discard(1); P.db.set_map_bad(1, False)
    (wl,), _, _ = P.nbest([14], [q], 1, [[]], ncand=3)               # query in map 1: its three key frames fill the loop list, merge fills first
    assert sorted(wl[0]) == [4, 5, 6] and len(wl[1]) == 3


@pytest.mark.parametrize("backend", BACKENDS)
def test_relocalisation_output_rules(lib, backend):
    """bestKF in another map is dropped; two entries electing one bestKF give one candidate at the first one's position; an entry exactly at
    0.75f * bestAccScore is not a candidate; cap_cand overflow with n_required"""
    # every key frame shares exactly word 1 with weight 0.5 on both sides: score exactly 0.5, so acc = 0.5 * (1 + neighbours) exactly
    q = (np.array([1, 2], np.int32), [0.5, 0.5])
    kf = lambda other: (np.array([1, other], np.int32), [0.5, 0.5])   # noqa: E731
    bows = [kf(10 + i) for i in range(8)]
    covis = [[1, 2, 3], [2, 3], [], [], [], [], [], []]
    P = small_pair(lib, backend, bows, maps=0, covis=covis)
    (w,), (e,), _ = P.reloc([1], [q], 0)
    assert e["best_acc"] == f32(2.0) and f32(1.5) in e["accs"] and e["at_threshold"] == 1 and w == [0], (w, e)
    # slot 4 scores higher than the rest and is elected by 5 and 6 (and itself): one candidate, at slot 4's own (earliest) position; 7 elects
    # slot 3 which lies in another map
    # (scores: 0.5 for [1, 2, x] with values .25 .25 .5; 1.0 for slot 4 = the query; 0.9 for slot 3 in map 1, elected by 7)
    bows2 = [(np.array([1, 2, 10 + i], np.int32), [0.25, 0.25, 0.5]) for i in range(8)]
    bows2[4] = (np.array([1, 2], np.int32), [0.5, 0.5])
    bows2[3] = (np.array([1, 2, 77], np.int32), [0.5, 0.4, 0.1])
    P2 = small_pair(lib, backend, bows2, maps=[0, 0, 0, 1, 0, 0, 0, 0], covis=[[1, 2], [], [0, 1], [], [], [4], [4], [3]])
    (w2,), (e2,), res = P2.reloc([1], [q], 0)
    # acc: 1.5 (0), .5, 1.5 (2), .9, 1.0, 1.5 -> 4, 1.5 -> 4 again, 1.4 -> 3 (other map); retained above 1.125
    assert e2["n_scored"] == 8 and e2["dups"] == 1 and e2["dropped_other_map"] == 1 and w2 == [0, 2, 4], (w2, e2)
    # overflow: 8 candidates, room for 3
    P3 = small_pair(lib, backend, bows, maps=0)
    (w3,), _, res3 = P3.reloc([1], [q], 0, cap_cand=3)
    assert len(w3) == 8 and to_host(res3["n_required"])[0] == 8 and to_host(res3["n_cand"])[0] == 3
    with pytest.raises(OrbHipError) as ei:
        P3.db.check_overflow(res3)
    assert ei.value.code == ORB_E_CAPACITY
    P.db.check_overflow(res)


@pytest.mark.parametrize("backend", BACKENDS)
def test_chained_with_vocabulary_transform(lib, backend):
    """ORBVocabulary.transform writes the BowVectors straight into database rows and into the query slab (zero-copy add)"""
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (400, 32), dtype=np.uint8)
    V = ORBVocabulary(synth_vocabulary(3, 10, 3, sample_desc=base), lib=lib)
    n_kf, cap = 12, 160

    def frames(count):
        desc, n = np.zeros((count, cap, 32), np.uint8), np.zeros(count, np.int32)
        for b in range(count):
            pick = (np.arange(120) + 25 * b) % 400
            d = base[pick].copy()
            flip = rng.integers(0, 256, (len(d), 3))
            for j in range(3):
                d[np.arange(len(d)), flip[:, j] >> 3] ^= (1 << (flip[:, j] & 7)).astype(np.uint8)
            desc[b, :len(d)] = d; n[b] = len(d)
        return desc, n
    P = Pair(lib, backend, n_kf, cap, n_rows=4)

    def dev(a):
        if backend == "emu":
            return a
        import torch
        return torch.from_numpy(a).to("cuda:0")
    desc, n = frames(n_kf)
    V.transform(dev(desc), dev(n), bv_out=P.db.rows(0, n_kf))
    P.h_word, P.h_val, P.h_n = (to_host(x).copy() for x in (P.db.bv_word, P.db.bv_value, P.db.bv_n))
    assert P.h_n.min() > 30
    P.add(list(range(n_kf)), [0] * 8 + [1] * 4)
    P.set_covisibles(list(range(n_kf)), [[(i + 1) % n_kf, (i - 1) % n_kf] for i in range(n_kf)])
    qd, qn = frames(4)
    V.transform(dev(qd), dev(qn), bv_out=P.qs)
    qw, qv, qc = (to_host(P.qs[k]) for k in ("bv_word", "bv_value", "bv_n"))
    qb = [(qw[r, :qc[r]].copy(), [float(x) for x in qv[r, :qc[r]]]) for r in range(4)]
    w, log, _ = P.reloc([1, 2, 3, 4], qb, 0, q_bows=P.qs)
    assert sum(len(x) for x in w) >= 4 and all(e["n_scored"] >= 1 for e in log)
    w, log, _ = P.nbest([1, 2, 3, 4], qb, 0, [[], [0], [], [1, 2]], q_bows=P.qs)
    assert sum(len(a) + len(b) for a, b in w) >= 4


@pytest.mark.parametrize("backend", BACKENDS)
def test_argument_errors(lib, backend):
    """ORB_E_INVALID without a launch; the wrapper refuses id 0 and a non-increasing id"""
    P = small_pair(lib, backend, [simple_bow([1, 2, 3])] * 3)
    db = P.db
    with pytest.raises(OrbHipError) as ei:
        db.set_queries(db.make_queries("reloc", 1), [0], 0)
    assert ei.value.code == ORB_E_INVALID
    db.set_queries(db.make_queries("reloc", 1), [7], 0)
    for ids in ([7], [3], [9, 9]):
        with pytest.raises(OrbHipError):
            db.set_queries(db.make_queries("reloc", len(ids)), ids, 0)
    Qp = db.set_queries(db.make_queries("place", 1), [7], 0)      # the families count separately
    with pytest.raises(OrbHipError):
        db.DetectNBestCandidates(Qp, P.qs, 0)
    with pytest.raises(OrbHipError):
        db.DetectNBestCandidates(Qp, P.qs, 65)
    from orbhip._lib import ptr as _ptr
    L = db._L
    Q = db.set_queries(db.make_queries("reloc", 1), [20], 0)
    out = db.DetectRelocalizationCandidates(Q, P.qs)
    state = [to_host(x).copy() for x in (db.reloc_query, db.reloc_score)]
    ws = db._workspace(1)

    def reloc_rc(view, bows, cap_cand=4, cand=out["cand"], work=ws):
        import ctypes as C
        return L.bowdb_detect_relocalization_candidates(C.byref(view), _ptr(Q.records), 1, C.byref(bows), _ptr(cand), cap_cand, _ptr(out["n_cand"]),
                                                        _ptr(out["n_required"]), None, _ptr(work), None)

    def nbest_rc(view, bows, ncand):
        import ctypes as C
        o = db.DetectNBestCandidates(Qp, P.qs, 3)
        return L.bowdb_detect_n_best_candidates(C.byref(view), _ptr(Qp.records), 1, C.byref(bows), None, 0, ncand, _ptr(o["loop"]), _ptr(o["n_loop"]),
                                                _ptr(o["merge"]), _ptr(o["n_merge"]), None, _ptr(ws), None)
    good_v, good_b = db._view(), db._bows(P.qs)
    bad = []
    v = db._view(); v.scoring = 1; bad.append(reloc_rc(v, good_b))
    v = db._view(); v.cap_f = 4097; bad.append(reloc_rc(v, good_b))
    v = db._view(); v.bv_value = None; bad.append(reloc_rc(v, good_b))
    v = db._view(); v.place_score = None; bad.append(reloc_rc(v, good_b))
    b = db._bows(P.qs); b.cap_q = 4097; bad.append(reloc_rc(good_v, b))
    b = db._bows(P.qs); b.q_n = None; bad.append(reloc_rc(good_v, b))
    bad.append(reloc_rc(good_v, good_b, cap_cand=-1))
    bad.append(reloc_rc(good_v, good_b, cand=None))
    bad.append(reloc_rc(good_v, good_b, work=None))
    bad.append(nbest_rc(good_v, good_b, 0))
    bad.append(nbest_rc(good_v, good_b, 65))
    assert bad == [ORB_E_INVALID] * len(bad), bad
    assert all(np.array_equal(a, to_host(x)) for a, x in zip(state, (db.reloc_query, db.reloc_score)))
    assert isinstance(good_v, View) and isinstance(good_b, QueryBows) and L.bowdb_workspace_bytes(3, 1) > 0


@pytest.mark.gpu
def test_graph_capture_replay_hip(hip_lib):
    """both calls captured on one stream and replayed after the query records were rewritten in place == plain calls on a second copy"""
    import torch
    A, rng, bows = build_random_pair(hip_lib, "hip", 21, 600, 20000, 150)
    B, _, _ = build_random_pair(hip_lib, "hip", 21, 600, 20000, 150)
    NQ = 4
    qs = query_sequence(rng, bows, 20000, 4 * NQ, A.cap_q)
    qb = [b for _, b in qs]
    conn = [[s] for s, _ in qs]
    A.load_queries(qb[:NQ])
    db = A.db
    Qr, Qp = db.make_queries("reloc", NQ), db.make_queries("place", NQ, cap_conn=16)
    db.set_queries(Qr, [1, 2, 3, 4], 0)
    db.set_queries(Qp, [1, 2, 3, 4], 0, conn=conn[:NQ])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):      # warm-up: workspace and outputs exist afterwards
        r_out = db.DetectRelocalizationCandidates(Qr, A.qs, 16)
        n_out = db.DetectNBestCandidates(Qp, A.qs, 3)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        db.DetectRelocalizationCandidates(Qr, A.qs, 16, out=r_out)
        db.DetectNBestCandidates(Qp, A.qs, 3, out=n_out)
    torch.cuda.synchronize()
    # B: the same history with plain calls (warm-up queries, then the new ones); the capture itself runs nothing
    B.reloc([1, 2, 3, 4], qb[:NQ], 0)
    B.nbest([1, 2, 3, 4], qb[:NQ], 0, conn[:NQ])
    A.load_queries(qb[NQ:2 * NQ])
    maps2 = [A.kfs[s_].map for s_, _ in qs[NQ:2 * NQ]]      # each query in the map of the key frame it was drawn near
    db.set_queries(Qr, [11, 12, 13, 14], maps2)
    db.set_queries(Qp, [11, 12, 13, 14], maps2, conn=conn[NQ:2 * NQ])
    for t in list(r_out.values()) + list(n_out.values()):
        if hasattr(t, "fill_"):
            t.fill_(90)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    wr, _, br = B.reloc([11, 12, 13, 14], qb[NQ:2 * NQ], maps2, cap_cand=16)
    wn, _, bn = B.nbest([11, 12, 13, 14], qb[NQ:2 * NQ], maps2, conn[NQ:2 * NQ])
    assert sum(len(w) for w in wr) >= 2 and sum(len(l) + len(m) for l, m in wn) >= 2
    for k in ("cand", "n_cand", "n_required", "stats"):
        a, b = to_host(r_out[k]), to_host(br[k])
        if k == "cand":
            nc = to_host(br["n_cand"])
            assert all(np.array_equal(a[i, :nc[i]], b[i, :nc[i]]) for i in range(NQ))
        else:
            assert np.array_equal(a, b), k
    for k in ("loop", "n_loop", "merge", "n_merge", "stats"):
        assert np.array_equal(to_host(n_out[k]), to_host(bn[k])), k
    for fam in ("reloc", "place"):
        for x in ("query", "score"):
            a, b = to_host(getattr(A.db, fam + "_" + x)), to_host(getattr(B.db, fam + "_" + x))
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (fam, x)
