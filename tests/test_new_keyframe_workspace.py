"""The workspace of the new-key-frame entry points (include/orbhip.h "New key frame"): orbm_newkf_workspace_bytes against the layout walked
here, and both entry points on a buffer of exactly that size with a guarded tail (tests/test_workspace_guard.py): nothing is written behind it."""
import pytest

from devarrays import BACKENDS, lib  # noqa: F401
from orbhip._abi import NEWKF_R_FLAGS
from orbhip.new_keyframe import NewKeyFrame
from test_new_keyframe import (KF, MP, SF, World, flatten, host, recent_arrays, restate_cull, restate_process, upload)
from test_workspace_guard import assert_tail_intact, guarded


@pytest.mark.parametrize("backend", BACKENDS)
def test_workspace_bytes(lib, backend):
    """hdr int32[8] | rank int32[n_kf] | first, mark int32[n_mp] | blk int32[ceil(n_mp / 256) + 1] | best int32[n_mp] | status uint32[n_mp] |
    sel int32[cap_feat], every section padded to 16 bytes"""
    pad = lambda n: (n + 15) & ~15   # noqa: E731
    for n_kf, n_mp, cap_feat in [(0, 0, 1), (1, 1, 1), (5, 3, 7), (31, 6001, 1000), (7, 256, 255), (3, 257, 257), (1025, 1, 2), (0, 513, 65535)]:
        secs = [32, pad(4 * n_kf)] + [pad(4 * n_mp)] * 2 + [pad(4 * ((n_mp + 255) // 256 + 1))] + [pad(4 * n_mp)] * 2 + [pad(4 * cap_feat)]
        assert lib.orbm_newkf_workspace_bytes(n_kf, n_mp, cap_feat) == sum(secs) and sum(secs) % 16 == 0, (n_kf, n_mp, cap_feat)
    assert lib.orbm_newkf_workspace_bytes(-1, 1, 1) == 0 and lib.orbm_newkf_workspace_bytes(1, -1, 1) == 0
    assert lib.orbm_newkf_workspace_bytes(1, 1, 0) == 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_both_entry_points_leave_the_tail(lib, backend):
    """7 features over 261 points in 3 key frames (odd counts: every section ends in padding, the points span two blocks), on guarded buffers
    of exactly orbm_newkf_workspace_bytes; the codes are the restatement's, so the sections do not overlap either"""
    n_mp = 261
    kfs = [KF(list(range(n_mp))), KF(list(range(n_mp))), KF([260, 3, None, 3, 259, 0, 1], id=110)]
    mps = [MP((0.01 * p, 0, 5), obs={0: p, 1: p}, found=p % 3, visible=4, first=108 + p % 3) for p in range(n_mp)]
    W = World(kfs, mps, [2, 0, 1])
    view, kk = flatten(W)
    dv, dk = upload(view, kk, backend)
    nk = NewKeyFrame(SF, 16, lib=lib)
    rec, n_rec = recent_arrays([5, 6, 7, 260], 16, backend)
    nbytes = lib.orbm_newkf_workspace_bytes(3, n_mp, 7)
    work = guarded(nbytes, backend)
    out = nk.ProcessNewKeyFrame(dv, dk, 2, 7, 600, rec, n_rec, work=work)
    assert_tail_intact(work, nbytes, backend)
    R = restate_process(W, 2, [5, 6, 7, 260], 16, 600)
    assert host(out["code"]).tolist() == R.code and host(out["result"])[NEWKF_R_FLAGS] == 0 and host(out["sel"])[:5].tolist() == R.sel
    # the culling sizes its own walk with cap_feat = 1
    nbytes = lib.orbm_newkf_workspace_bytes(3, n_mp, 1)
    work = guarded(nbytes, backend)
    dv, dk = upload(view, kk, backend)
    out = nk.MapPointCulling(dv, dk, 2, rec, n_rec, 600, work=work)
    assert_tail_intact(work, nbytes, backend)
    Rc = restate_cull(W, 2, R.recent, 600)
    assert host(out["code"])[:len(R.recent)].tolist() == Rc.code and host(out["culled"])[:len(Rc.culled)].tolist() == Rc.culled
