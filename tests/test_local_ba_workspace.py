"""The workspace of orbm_lba_window_build / orbm_lba_window_apply: its size against the section table of csrc/orbm_localba.hip, and nothing
written behind it (a buffer of orbm_lba_workspace_bytes + 4096 whose tail holds a byte pattern, as tests/test_workspace_guard.py does for
the other steps).  The shapes are odd, so that every section is padded."""
import numpy as np
import pytest

from devarrays import BACKENDS, lib  # noqa: F401
from test_local_ba import CAM, INV_SIGMA2, SF, LocalBA, chain_world, flatten, restate_build, set_dev, upload
from test_workspace_guard import assert_tail_intact, guarded


def pad16(n):
    return (n + 15) & ~15


def table(n_kf, n_mp, n_obs, n_rows, cap_conn, cap_p, cap_l, cap_e):
    """the sections of lb_work_layout in bytes, each padded to 16"""
    words = [32, n_kf, n_kf, cap_conn + 1, cap_conn + 2, n_mp, n_rows, n_mp, n_mp, n_kf, n_kf]          # hdr .. pcount
    tail = [n_mp, (n_mp + 255) // 256 + 1, n_mp, n_mp, cap_l]                                             # ndead, blk, best, status, sel
    return sum(pad16(4 * w) for w in words) + pad16(cap_e) + pad16(n_obs) + sum(pad16(4 * w) for w in tail)


@pytest.mark.parametrize("sizes", [(5, 7, 19, 23, 3, 4, 6, 9), (1, 1, 1, 1, 1, 1, 1, 1), (0, 0, 0, 0, 1, 1, 1, 1), (33, 257, 1021, 999, 40, 231, 300, 1300)])
def test_workspace_bytes(emu_lib, sizes):
    n = emu_lib.orbm_lba_workspace_bytes(*sizes)
    assert n == table(*sizes) and n % 16 == 0


def test_workspace_bytes_out_of_range(emu_lib):
    ok = [5, 7, 19, 23, 3, 4, 6, 9]
    for i in range(8):
        bad = list(ok)
        bad[i] = -1 if i < 4 else 0
        assert emu_lib.orbm_lba_workspace_bytes(*bad) == 0
    # (cap_conn + 1) * n_kf_mp_rows must stay an int: the feature positions of the local key frames are summed in one
    assert emu_lib.orbm_lba_workspace_bytes(5, 7, 19, 1 << 20, (1 << 11) - 2, 4, 6, 9) > 0
    assert emu_lib.orbm_lba_workspace_bytes(5, 7, 19, 1 << 20, (1 << 11) - 1, 4, 6, 9) == 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_guarded_tail(lib, backend):
    """both calls on a workspace with a guarded tail: the last section (the refresh's selection, cap_l words) ends the buffer"""
    W, cur = chain_world(5, fixed_kf=(0,))
    view, kfs, recs = flatten(W)
    B = restate_build(W, recs, cur, 0, (99, 99, 999))
    caps = (B.n_poses + 1, B.n_points + 2, B.n_edges + 3)
    dv, dk = upload(view, kfs, backend)
    ba = LocalBA(INV_SIGMA2, SF, CAM, *caps, lib=lib)
    nbytes = lib.orbm_lba_workspace_bytes(len(W.kfs), len(W.mps), len(view["obs"]), len(view["kf_mp"]), kfs["ordered_kf"].shape[1], *caps)
    work = guarded(nbytes, backend)
    win = ba.Build(dv, dk, cur, 0, work=work)
    assert win["work"] is work
    assert_tail_intact(work, nbytes, backend)
    chi2 = np.ones(B.n_edges)
    chi2[::7] = 50.0
    set_dev(win["chi2"], chi2, backend); set_dev(win["depth"], np.ones(B.n_edges), backend)
    out = ba.Apply(dv, dk, win)
    assert win["work"] is work
    assert_tail_intact(work, nbytes, backend)
    from devarrays import to_host
    assert int(to_host(out["result"])[1]) == len(chi2[::7])
