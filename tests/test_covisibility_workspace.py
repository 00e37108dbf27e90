"""The workspace of the covisibility entry points (include/orbhip.h "Covisibility graph"): orbm_covis_workspace_bytes against the layout walked
here, and both entry points on a buffer of exactly that size with a guarded tail (tests/test_workspace_guard.py): nothing is written behind it."""
import numpy as np
import pytest

from devarrays import BACKENDS, lib, to_dev_plain  # noqa: F401
from orbhip._abi import CULL_EVENT_DTYPE
from orbhip.covisibility import CovisibilityGraph
from test_covisibility import INIT_NONE, World, check_store, erase_connections, flatten, rec_dev, shared, sync, update_connections, upload
from test_workspace_guard import assert_tail_intact, guarded


@pytest.mark.parametrize("backend", BACKENDS)
def test_workspace_bytes(lib, backend):
    """hdr int32[8] | cnt int32[n_list][n_kf] | mode uint32[n_kf] | stamp, erased_at, rank_of int32[n_kf], every section padded to 16 bytes"""
    pad = lambda n: (n + 15) & ~15   # noqa: E731
    for n_kf, n_list in [(0, 0), (1, 1), (5, 3), (7, 0), (64, 70), (65, 1), (300, 70), (101, 100), (3, 5), (0, 9)]:
        secs = [32, pad(4 * n_list * n_kf)] + [pad(4 * n_kf)] * 4
        assert lib.orbm_covis_workspace_bytes(n_kf, n_list) == sum(secs) and sum(secs) % 16 == 0, (n_kf, n_list)
    assert lib.orbm_covis_workspace_bytes(-1, 1) == 0 and lib.orbm_covis_workspace_bytes(1, -1) == 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_both_entry_points_leave_the_tail(lib, backend):
    """an update of 3 list entries over 7 key frames (odd counts: every section ends in padding), then an erase, on guarded buffers of exactly
    orbm_covis_workspace_bytes; the results are the restatement's, so the sections do not overlap either"""
    kfp, n_mp = shared([16, 17, 3, 15, 20, 14])
    W0 = World(kfp, n_mp, rng=np.random.default_rng(5))
    view, ckf, st = flatten(W0)
    dv, dckf, ds = upload(view, ckf, st, backend)
    G = CovisibilityGraph(ds, dckf, lib=lib)
    lst = [0, 5, 2]
    nbytes = lib.orbm_covis_workspace_bytes(len(W0.kfs), len(lst))
    work = guarded(nbytes, backend)
    G.UpdateConnections(dv, to_dev_plain(np.asarray(lst, np.int32), backend), INIT_NONE, work=work)
    assert_tail_intact(work, nbytes, backend)
    W = W0   # (flatten gave W0 its row model)
    for a in lst:
        update_connections(W, a, INIT_NONE)
    check_store(W, view, ckf, st, dv, dckf, ds)
    # the erase sizes its own walk with n_list = 0
    W.rebuilt = set()
    view, ckf, st = flatten(W)
    dv, dckf, ds = upload(view, ckf, st, backend)
    G = CovisibilityGraph(ds, dckf, lib=lib)
    ev = np.zeros(2, CULL_EVENT_DTYPE)
    ev["kf"] = [5, 0]
    nbytes = lib.orbm_covis_workspace_bytes(len(W.kfs), 0)
    work = guarded(nbytes, backend)
    G.EraseConnections(dv, rec_dev(ev, backend), to_dev_plain(np.asarray([2], np.int32), backend), work=work)
    sync(backend)
    assert_tail_intact(work, nbytes, backend)
    erase_connections(W, [(5, True), (0, True)])
    check_store(W, view, ckf, st, dv, dckf, ds)
