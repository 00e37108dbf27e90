"""The one part of row N2 that is pinned to the REFERENCE compiled here (round-4 verdict, item 7): oracle/_ref/libdbow_ref.so = the reference's
Thirdparty/DBoW2/DBoW2/{BowVector,FeatureVector}.cpp compiled as they lie (`make -C oracle _ref`, run by build() where the reference tree exists;
shim oracle/dbow_ref_shim.cc).  oracle/bow_oracle.cpp restates BowVector::addWeight / addIfNotExist / normalize (BowVector.cpp:34-84) and
FeatureVector::addFeature (FeatureVector.cpp:28-41) inside its transform(); here the per-feature (word, weight, node) sequences the oracle's descent
produces are replayed through the reference's own classes and the resulting doubles / index lists must equal the oracle's outputs bit for bit.
Where the library was not built, the reference's answers to the same calls come from tests/golden/dbow_ref.npz, recorded from the library by
`tests/golden/make_golden.py dbow_ref`; where it was built, its answers must also equal that recording.  What this does NOT pin: the descent
(FORB::distance, the tree walk of TemplatedVocabulary.h) and the size-division of the not-normalised scorings — both live in headers that need
OpenCV."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import oracle_lib as O
from orbhip.bow import BINARY, DOT_PRODUCT, IDF, L1_NORM, L2_NORM, TF, TF_IDF, synth_vocabulary
from test_matcher_parity import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libdbow_ref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dbow_ref.npz")


def _load_lib():
    if not os.path.exists(REF_SO):
        return None
    L = C.CDLL(REF_SO)
    L.dbr_bowvector.restype = C.c_int
    L.dbr_bowvector.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.dbr_featurevector.restype = C.c_int
    L.dbr_featurevector.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return L


class RefDBoW:
    """The compiled reference's BowVector / FeatureVector, or their recorded answers.  Every call carries a name: a recorded answer is handed out
    only for the inputs it was recorded with (sha256), and when the library is there as well its answer must equal the recording bit for bit.
    With `record` (a dict) the library's answers are collected for tests/golden/dbow_ref.npz instead."""

    def __init__(self, lib, golden, record=None):
        self.lib, self.golden, self.record = lib, golden, record

    def _answer(self, key, inputs, live, n_out):
        sha = np.frombuffer(hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in inputs)).digest(), np.uint8)
        if self.record is not None:
            self.record[key + ".sha"] = sha
            for i, a in enumerate(live):
                self.record["%s.%d" % (key, i)] = a
            return live
        assert key + ".sha" in self.golden.files, "%s: no recorded answer in tests/golden/dbow_ref.npz (tests/golden/make_golden.py dbow_ref)" % key
        assert np.array_equal(self.golden[key + ".sha"], sha), "%s: the inputs differ from the recorded call" % key
        rec = [self.golden["%s.%d" % (key, i)] for i in range(n_out)]
        if live is None:
            return rec
        assert all(a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(live, rec)), \
            "%s: the compiled reference and tests/golden/dbow_ref.npz disagree" % key
        return live

    def bow(self, key, ids, vals, mode, norm):
        ids = np.ascontiguousarray(ids, np.uint32); vals = np.ascontiguousarray(vals, np.float64)
        live = None
        if self.lib is not None:
            oi = np.zeros(len(ids) + 1, np.uint32); ov = np.zeros(len(ids) + 1)
            n = self.lib.dbr_bowvector(_p(ids), _p(vals), len(ids), mode, norm, _p(oi), _p(ov), len(oi))
            assert n >= 0
            live = [oi[:n], ov[:n]]
        return self._answer(key, (ids, vals, np.array([mode, norm], np.int32)), live, 2)

    def featurevector(self, key, nodes, feat, n_on, n_os, n_of):
        """-> (k, node ids [n_on], node starts [n_os], feature indices [n_of])"""
        nodes = np.ascontiguousarray(nodes, np.uint32); feat = np.ascontiguousarray(feat, np.uint32)
        live = None
        if self.lib is not None:
            on = np.zeros(n_on, np.uint32); os_ = np.zeros(n_os, np.int32); of = np.zeros(n_of, np.uint32)
            k = self.lib.dbr_featurevector(_p(nodes), _p(feat), len(nodes), _p(on), _p(os_), _p(of), n_on)
            live = [np.array([k], np.int32), on, os_, of]
        k, on, os_, of = self._answer(key, (nodes, feat, np.array([n_on, n_os, n_of], np.int32)), live, 4)
        return int(k[0]), on, os_, of


def _ref():
    lib = _load_lib()
    golden = np.load(GOLDEN) if os.path.exists(GOLDEN) else None
    if golden is None:
        pytest.fail("tests/golden/dbow_ref.npz is missing (tests/golden/make_golden.py dbow_ref)")
    return RefDBoW(lib, golden)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def known_answers(R):
    i, v = R.bow("ka_add", [5, 2, 5, 9, 2], [1.0, 2.0, 0.5, 4.0, 0.25], 0, -1)              # addWeight accumulates, std::map order
    assert i.tolist() == [2, 5, 9] and v.tolist() == [2.25, 1.5, 4.0]
    i, v = R.bow("ka_first", [5, 2, 5, 9, 2], [1.0, 2.0, 0.5, 4.0, 0.25], 1, -1)            # addIfNotExist keeps the first
    assert i.tolist() == [2, 5, 9] and v.tolist() == [2.0, 1.0, 4.0]
    i, v = R.bow("ka_l1", [1, 2], [3.0, -1.0], 0, 0)                                          # L1: sum of |v|
    assert v.tolist() == [0.75, -0.25]
    i, v = R.bow("ka_l2", [1, 2], [3.0, 4.0], 0, 1)                                           # L2
    assert v.tolist() == [3.0 / 5.0, 4.0 / 5.0]
    i, v = R.bow("ka_zero", [1, 2], [0.0, 0.0], 0, 0)                                         # norm 0: left alone (BowVector.cpp:79)
    assert v.tolist() == [0.0, 0.0]
    nodes = np.array([7, 3, 7, 3, 1], np.uint32); feat = np.array([0, 1, 2, 3, 4], np.uint32)
    k, on, os_, of = R.featurevector("ka_fv", nodes, feat, 6, 7, 5)
    assert k == 3 and on[:3].tolist() == [1, 3, 7] and os_[:4].tolist() == [0, 1, 3, 5] and of.tolist() == [4, 1, 3, 0, 2]


def accumulation(R, scoring, weighting):
    S = scene()
    for seed, desc in ((0, S["da"]), (1, S["db"]), (2, np.concatenate([S["da"], S["db"], S["da"][:50]]))):
        key = "acc_%d_%d_%d" % (scoring, weighting, seed)
        blob = synth_vocabulary(seed, 6, 3, scoring, weighting, stop_frac=0.05, sample_desc=np.concatenate([S["da"], S["db"]]))
        ov = O.OracleVocabulary(blob)
        o = ov.transform(desc, levelsup=2)
        n = len(desc)
        keep = o["weight"][:n] > 0                                                      # TemplatedVocabulary.h:1167 `if(w > 0)`
        ids, w, nid = o["word_id"][:n][keep], o["weight"][:n][keep], o["node_id"][:n][keep]
        feat = np.nonzero(keep)[0].astype(np.uint32)
        assert keep.sum() > 50 and (~keep).sum() > 0                                    # stop words occur
        mode = 0 if weighting in (TF, TF_IDF) else 1                                    # TemplatedVocabulary.h:1160 / :1189
        norm = {L1_NORM: 0, L2_NORM: 1}.get(scoring, -1)                                # mustNormalize (ScoringObject.h)
        ri, rv = R.bow(key + "_bv", ids, w, mode, norm)
        m = o["bv_n"]
        if norm < 0 and mode == 0:                                                      # the division by v.size() of TemplatedVocabulary.h:1177-1184 is not in BowVector.cpp
            rv = rv / float(len(rv))
        assert m == len(ri) and np.array_equal(o["bv_word"][:m].astype(np.uint32), ri)
        assert np.array_equal(o["bv_value"][:m].view(np.uint64), rv.view(np.uint64)), "BowVector doubles differ from the compiled reference"
        nn = np.ascontiguousarray(nid, np.uint32)
        k, on, os_, of = R.featurevector(key + "_fv", nn, feat, len(nn) + 1, len(nn) + 2, len(nn) + 1)
        assert k == o["fv_n_nodes"] and np.array_equal(on[:k], o["fv_node_id"][:k].astype(np.uint32))
        assert np.array_equal(os_[:k + 1], o["fv_node_start"][:k + 1]) and np.array_equal(of[:len(nn)], o["fv_feat_idx"][:len(nn)].astype(np.uint32))


SCORING_WEIGHTING = [(L1_NORM, TF_IDF), (L2_NORM, TF_IDF), (L1_NORM, TF), (L1_NORM, IDF), (L2_NORM, BINARY), (DOT_PRODUCT, TF_IDF)]


def test_reference_bowvector_known_answers():
    """the compiled reference itself on hand-made sequences (so a broken build of it cannot hide behind an equally broken restatement)"""
    known_answers(_ref())


@pytest.mark.parametrize("scoring,weighting", SCORING_WEIGHTING)
def test_oracle_accumulation_equals_compiled_reference(scoring, weighting):
    """ORBvoc's own combination (TF_IDF + L1_NORM, TemplatedVocabulary.h:1442-1480 header of the stock file) and the other weighting / norm branches:
    the oracle's per-feature sequence through the reference's BowVector / FeatureVector == the oracle's own BowVector / FeatureVector, bitwise."""
    accumulation(_ref(), scoring, weighting)


def record_reference_answers():
    """tests/golden/make_golden.py dbow_ref: every call above, answered by the compiled reference -> dict for np.savez_compressed"""
    lib = _load_lib()
    assert lib is not None, "oracle/_ref/libdbow_ref.so is not built (make -C oracle _ref)"
    rec = {}
    R = RefDBoW(lib, None, record=rec)
    known_answers(R)
    for sc, wt in SCORING_WEIGHTING:
        accumulation(R, sc, wt)
    return rec
