"""The six *_workspace_bytes functions over a table of shapes (tests/golden/workspace_bytes.json).

A workspace's size is its layout function walked with a null base; the table was recorded before the layouts were written
that way and pins every size: zero and negative arguments, odd counts (per-section padding), and for lba_lm_workspace_bytes both sides of every
condition that adds a section.  The emulated build reports 256 compute units, as an MI355X does, so one table serves both backends.
`python tests/golden/make_golden.py workspace_bytes` rewrites the table from the emulated build."""
import ctypes as C
import json
import os

import pytest

from devarrays import BACKENDS, lib  # noqa: F401  (lib: the fixture of the tests parametrised over BACKENDS)
from orbhip._abi import LbaProblem, LibaProblem

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.json")

# lba_lm_workspace_bytes: (batch, cap_p, cap_l, cap_e); cap_p None = a null problem
LBA = [(1, None, 0, 0), (0, 6, 300, 2000), (-1, 6, 300, 2000), (3, 5, 7, 13)]
# cholL / cholY / cholX up to 48 windows per call; the panel in the workspace from 177 key frames; neither beyond 1 GB of factors (48 x 300)
LBA += [(b, p, 300, 2000) for b in (1, 48, 49) for p in (6, 176, 177)] + [(1, 300, 300, 2000), (48, 300, 300, 2000)]
# split Schur rows: a row of a 2- / 3-pose window is split once cap_e reaches 512 x rows (the size takes the most slices of any row count)
LBA += [(1, p, 40, e) for p in (2, 3) for e in (511, 512, 1023, 1024, 1100, 1535, 1536, 4096)]
# ... never once the batch alone has a row per compute unit; only one-row systems at half of that; 64 MB of partial rows at most
LBA += [(257, 3, 40, 5000), (128, 3, 40, 5000), (1, 250, 300, 200000)]
# liba_workspace_bytes: (batch, cap_kf, cap_l, cap_e, cap_i, max_free); batch 0 sizes one window, an invalid problem 0
LIBA = [(1, 8, 250, 1500, 6, 6), (2, 5, 7, 13, 3, 3), (3, 5, 7, 13, 0, 1), (0, 5, 7, 13, 3, 3), (-1, 5, 7, 13, 3, 3), (1, 5, 7, 13, 3, 0),
        (1, 5, 7, 13, 3, 33), (1, 40, 3000, 20000, 25, 32)]
BOWDB = [(5, 3), (5, 1), (7, 2), (0, 0), (0, 1), (1, 0), (-1, 1), (5, -1), (1000, 4)]                   # (n_slots, n_queries)
LOCAL_MAP = [(5, 7, 2), (6, 7, 1), (7, 7, 1), (8, 7, 1), (0, 0, 1), (5, 7, 0), (-1, 1, 1), (1, -1, 1), (5, 7, -1), (10, 100, 2)]   # (n_kf, n_mp, batch)
SEARCH = [(3, 5), (1, 1), (4, 7), (5, 300), (8, 1000), (0, 5), (3, 0)]                                   # (batch, cap_q)
SIM3 = [(2, 100, 3), (1, 100, 1), (3, 100, 300), (0, 100, 5), (3, 100, 0), (-1, 100, 5), (2, 100, -1)]   # (batch, cap_n, cap_its)


def workspace_bytes_table(L):
    """-> {function: [[arguments..., bytes], ...]} as `L` answers now"""
    def lba(batch, cap_p, cap_l, cap_e):
        if cap_p is None:
            return L.lba_lm_workspace_bytes(None, batch)
        P = LbaProblem(*[0] * 11, cap_p, cap_l, cap_e, 1, 1.0, 1.0)   # sizes read the capacities only
        return L.lba_lm_workspace_bytes(C.byref(P), batch)

    def liba(batch, cap_kf, cap_l, cap_e, cap_i, max_free):
        P = LibaProblem(*[8] * 9, cap_kf, cap_l, cap_e, cap_i, 1, max_free, 1.0, 1.0)   # (a valid problem has its arrays; none is read)
        return L.liba_workspace_bytes(C.byref(P), batch)
    rows = {"lba_lm_workspace_bytes": (lba, LBA), "liba_workspace_bytes": (liba, LIBA), "bowdb_workspace_bytes": (L.bowdb_workspace_bytes, BOWDB),
            "orbm_local_map_workspace_bytes": (L.orbm_local_map_workspace_bytes, LOCAL_MAP),
            "orbm_search_workspace_bytes": (L.orbm_search_workspace_bytes, SEARCH), "orbm_sim3_workspace_bytes": (L.orbm_sim3_workspace_bytes, SIM3)}
    return {name: [list(a) + [int(f(*a))] for a in shapes] for name, (f, shapes) in rows.items()}


@pytest.mark.parametrize("backend", BACKENDS)
def test_workspace_sizes_match_the_recorded_table(lib, backend):
    with open(TABLE) as f:
        want = json.load(f)
    got = workspace_bytes_table(lib)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], (name, [(g, w) for g, w in zip(got[name], want[name]) if g != w])
