"""The launch plans of the LM loop's reduced-system solve, each run on its own against a higher-precision reference.

lba_optimize picks its Cholesky from a lattice of plans (lm_plan in csrc/lba_build.hip): one launch per 32-column panel (few windows per call,
up to 544 unknowns), one workgroup per window with a 32-column or a 16-column LDS panel, or a 16-column panel in global memory.  The whole-loop
parity tests compare LM trajectories, where a factorisation that loses three digits still converges to the same poses; here the solve alone is
handed symmetric positive definite systems (lba_debug_solve_reduced: the launch code of lba_optimize, no LM around it) and judged by the scaled
residual  |H x - b|_inf / (|H|_inf |x|_inf + |b|_inf)  evaluated in numpy.longdouble.

Every case first asserts the plan it was written for (lba_debug_lm_plan): a threshold that moves makes the case fail, not test something else.

The bar.  The same systems go through numpy.linalg.solve (LAPACK, fp64) and the same residual; the kernel's residual may exceed the larger of
that and N 2^-53 (N unknowns: the backward error bound of a Cholesky factorisation grows with the dimension) by RESIDUAL_FACTOR.  The factor
pays for what the kernels do and LAPACK does not: reciprocal-square-root pivots, panel rows as products with an explicitly inverted diagonal
block, matrix-core summation orders.  It is the next power of two above twice the largest ratio measured on an MI355X over all cases of this
file (stage-3 notes, has the ratios per plan)."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
from orbhip.lba import HUBER_MONO, HUBER_STEREO, synth_window

LD = np.longdouble
RESIDUAL_FACTOR = 1.0      # largest ratio measured on an MI355X: 0.28 ("Stage 3: the solver plans on their own")
PER_PANEL, WG_NB32, WG_NB16, WG_NB16_GLOBAL = 0, 1, 2, 3
PLAN_NAMES = {PER_PANEL: "one launch per 32-column panel", WG_NB32: "one workgroup, 32-column LDS panel", WG_NB16: "one workgroup, 16-column LDS panel",
              WG_NB16_GLOBAL: "one workgroup, 16-column panel in global memory"}

# nfree: panel edges (6 free = 36 unknowns, the first size past one 32-column panel) | panel-width thresholds | the 512-thread backward layout
# (513 ... 544 unknowns wrap it; 91 is the first size back on one workgroup) | the LDS limit
SIZES = [1, 2, 3, 5, 6, 11, 16, 53, 54, 88, 89, 85, 86, 90, 91, 120, 176, 177]
KINDS = ["gram", "scaled", "ba"]


def solver(lib):
    """the two debug exports (not part of the public ABI: bound here, not in orbhip._abi)"""
    if not getattr(lib, "_lm_debug_bound", False):
        i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
        lib.lba_debug_lm_plan.restype = ctypes.c_int
        lib.lba_debug_lm_plan.argtypes = [ctypes.c_int] * 5 + [i32p]
        lib.lba_debug_solve_reduced.restype = ctypes.c_int
        lib.lba_debug_solve_reduced.argtypes = [ctypes.c_int] * 3 + [f64p, f64p, i32p, f64p, i32p]
        lib._lm_debug_bound = True
    return lib


def lm_plan(lib, batch, cap_p, cap_l, cap_e, max_free):
    """-> dict(chol, nb, pan_global, schur_nw, schur_g, row_cap, split_ws, step_ws)"""
    out = np.zeros(8, np.int32)
    rc = solver(lib).lba_debug_lm_plan(batch, cap_p, cap_l, cap_e, max_free, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert rc == 0, rc
    return dict(zip(("chol", "nb", "pan_global", "schur_nw", "schur_g", "row_cap", "split_ws", "step_ws"), (int(v) for v in out)))


def expected_chol_plan(batch, nfree):
    """what this file was written for, from the thresholds of csrc/lba_build.hip / dense_chol.inc at their default values"""
    n = 6 * nfree
    if batch <= 48 and n <= 544:
        return PER_PANEL
    if n > 1060:
        return WG_NB16_GLOBAL
    return WG_NB32 if 320 < n <= 528 else WG_NB16


def solve_reduced(lib, mats, rhs, max_free):
    """mats[b]: [n_b, n_b] symmetric, rhs[b]: [n_b] -> (x list, ok [batch]).  Only what the kernels may read is given: the lower triangle of the
    column-major system (S[c * ld + r], r >= c) and the first n_b entries; the other triangle and the padding up to 6 x max_free are NaN."""
    B, ld = len(mats), 6 * max_free
    H = np.full((B, ld, ld), np.nan)
    b = np.full((B, ld), np.nan)
    nfree = np.zeros(B, np.int32)
    for i, (m, r) in enumerate(zip(mats, rhs)):
        n = len(r)
        H[i, :n, :n] = np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], m, np.nan)   # C order [c, r]: kept where r >= c
        b[i, :n] = r
        nfree[i] = n // 6
    x = np.zeros((B, ld))
    ok = np.full(B, -1, np.int32)
    f64p, i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    rc = solver(lib).lba_debug_solve_reduced(B, max_free, max_free, H.ctypes.data_as(f64p), b.ctypes.data_as(f64p), nfree.ctypes.data_as(i32p),
                                             x.ctypes.data_as(f64p), ok.ctypes.data_as(i32p))
    assert rc == 0, rc
    return [x[i, :len(r)].copy() for i, r in enumerate(rhs)], ok


# ---- the reference: plain Cholesky in numpy.longdouble --------------------------------------------------------------------------------------
def chol_solve_longdouble(H, b):
    A, n = H.astype(LD), len(b)
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        assert d > 0, "the test system is not positive definite"
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(n, LD)
    for j in range(n):
        y[j] = (LD(b[j]) - L[j, :j] @ y[:j]) / L[j, j]
    x = np.zeros(n, LD)
    for j in range(n - 1, -1, -1):
        x[j] = (y[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    return x


def scaled_residual(H, x, b, equilibrate=False):
    """equilibrate: the residual of the same solution in the system scaled to a unit diagonal, (D^-1 H D^-1)(D x) = D^-1 b with D = sqrt(diag H) —
    the norm-wise residual of a badly scaled system is decided by its few largest rows, this one weighs every unknown alike"""
    Hl, xl, bl = H.astype(LD), np.asarray(x).astype(LD), b.astype(LD)
    if equilibrate:
        d = np.sqrt(np.diag(Hl))
        Hl, xl, bl = Hl / d[:, None] / d[None, :], xl * d, bl / d
    return float(np.abs(Hl @ xl - bl).max() / (np.abs(Hl).sum(1).max() * np.abs(xl).max() + np.abs(bl).max()))


# ---- the systems ------------------------------------------------------------------------------------------------------------------------------
_SYS, _REF = {}, {}


def ba_reduced_system(nfree):
    """The reduced camera system of a synthetic stereo window with `nfree` free key frames and one fixed one, as the LM loop forms it at its
    first trial: H_pp + lambda I - sum_l W_l (H_ll + lambda I)^-1 W_l^T from the oracle's buildSystem blocks, lambda = 1e-5 max diag (g2o's tau)."""
    w, cams = synth_window(900 + nfree, nfree + 1, 1, max(60, 12 * nfree), min(8, nfree + 1), "stereo")
    o = O.lba_build_system(w, cams, (HUBER_MONO, HUBER_STEREO))
    assert o["nfree"] == nfree
    n, nl = 6 * nfree, len(w["points"])
    Hpp, Hll = o["Hpp"][:nfree].reshape(nfree, 6, 6), o["Hll"].reshape(nl, 3, 3)
    lam = 1e-5 * max(np.abs(np.einsum("kii->ki", Hpp)).max(), np.abs(np.einsum("kii->ki", Hll)).max())
    W = np.zeros((n, nl, 3))
    h = w["pose_hidx"][w["edges"]["pose"]]
    for e in np.nonzero(h >= 0)[0]:
        W[6 * h[e]:6 * h[e] + 6, w["edges"]["point"][e]] = o["Hpl"][e].reshape(3, 6).T
    Dinv = np.linalg.inv(Hll + lam * np.eye(3))
    S = lam * np.eye(n) - np.einsum("ilr,lrs->ils", W, Dinv).reshape(n, -1) @ W.reshape(n, -1).T
    for k in range(nfree):
        S[6 * k:6 * k + 6, 6 * k:6 * k + 6] += Hpp[k]
    S = 0.5 * (S + S.T)
    bp = o["bp"][:nfree].reshape(n) - np.einsum("ils,ls->i", np.einsum("ilr,lrs->ils", W, Dinv), o["bl"])
    return S, bp


def system(kind, nfree):
    """-> (H [6 nfree, 6 nfree], b): gram = G G^T + nfree I;  scaled = D (G G^T + nfree I) D, D log-uniform over 1e-5 .. 1e5 (condition ~1e10, the
    shape a BA reduced system has between rotation and translation unknowns);  ba = ba_reduced_system.  A smaller system of the same kind inside a
    ragged batch is the leading principal block (positive definite with the whole)."""
    k = (kind, nfree)
    if k not in _SYS:
        n = 6 * nfree
        rng = np.random.default_rng(1000 * KINDS.index(kind) + nfree)
        if kind == "ba":
            H, b = ba_reduced_system(nfree)
        else:
            G = rng.normal(size=(n, n))
            H = G @ G.T + nfree * np.eye(n)
            if kind == "scaled":
                D = 10.0 ** rng.uniform(-5, 5, n)
                H = H * D[:, None] * D[None, :]
            H = 0.5 * (H + H.T)
            b = H @ rng.normal(size=n)
        H.setflags(write=False); b.setflags(write=False)
        _SYS[k] = (H, b)
    return _SYS[k]


def reference(kind, nfree, m):
    """the leading m-free-key-frame block of system(kind, nfree): (H, b, fp64 LAPACK residual), computed once"""
    k = (kind, nfree, m)
    if k not in _REF:
        H, b = system(kind, nfree)
        H, b = H[:6 * m, :6 * m], b[:6 * m]
        x = np.linalg.solve(H, b)
        _REF[k] = (H, b, (scaled_residual(H, x, b), scaled_residual(H, x, b, True)))
    return _REF[k]


def ragged(nfree, batch):
    """free key-frame counts of the batch's windows"""
    if batch == 1:
        return [nfree]
    if batch == 3:
        return [nfree, max(nfree - 1, 1), 1]
    vals = sorted({nfree, max(nfree - 1, 1), max((nfree + 1) // 2, 1), min(3, nfree), 1}, reverse=True)   # a handful, up to nfree: every value several times
    return [vals[i % len(vals)] for i in range(batch)]


def check_solve(lib, kind, nfree, batches, factor=RESIDUAL_FACTOR, plan_of=expected_chol_plan, tag="hip"):
    worst, by_batch = 0.0, {}
    for batch in batches:
        ms = ragged(nfree, batch)
        plan = lm_plan(lib, batch, nfree, 1, 0, nfree)
        want = plan_of(batch, nfree)
        print("[%s] %s nfree=%d batch=%d: plan %d (%s), panel width %d" % (tag, kind, nfree, batch, plan["chol"], PLAN_NAMES[plan["chol"]], plan["nb"]))
        assert plan["chol"] == want, "this case no longer takes plan '%s' but '%s'" % (PLAN_NAMES[want], PLAN_NAMES[plan["chol"]])
        assert plan["pan_global"] == (want == WG_NB16_GLOBAL) and plan["nb"] == (32 if want in (PER_PANEL, WG_NB32) else 16)
        refs = [reference(kind, nfree, m) for m in ms]
        xs, ok = solve_reduced(lib, [r[0] for r in refs], [r[1] for r in refs], nfree)
        assert (ok == 1).all(), ok
        first = {}
        for i, (m, (H, b, res_lapack)) in enumerate(zip(ms, refs)):
            if m in first:                                       # copies of one system inside a batch: the same bits
                assert np.array_equal(xs[i], xs[first[m]]), (batch, i, first[m])
                continue
            first[m] = i
            for eq in (False, True):     # the issue's residual, and the same bar on the equilibrated one (Cholesky's error bound is scaling-invariant)
                res = scaled_residual(H, xs[i], b, eq)
                bar = max(res_lapack[eq], 6 * m * 2.0 ** -53)
                print("    window %d (%d free)%s: residual %.3e, LAPACK %.3e, N 2^-53 %.3e -> ratio %.3f"
                      % (i, m, " equilibrated" if eq else "", res, res_lapack[eq], 6 * m * 2.0 ** -53, res / bar))
                worst = max(worst, res / bar)
                assert res <= factor * bar, (kind, nfree, batch, i, m, eq, res, bar)
        by_batch[batch] = xs[0]
    # the longdouble solve: the metric and the system are sound (its own residual is below fp64's resolution), and the forward error is reported
    H, b = system(kind, nfree)
    x_ref = chol_solve_longdouble(H, b)
    assert scaled_residual(H, x_ref, b) < 2.0 ** -53
    d = np.sqrt(np.diag(H))
    print("    equilibrated forward error vs longdouble: %s" % {bt: float(np.abs(d * (x - x_ref)).max() / np.abs(d * x_ref).max()) for bt, x in by_batch.items()})
    # the same system through two plans.  Two backward-stable solvers agree to cond x eps, and for a Cholesky factorisation the condition that counts
    # is the one of the system scaled to a unit diagonal (van der Sluis): the difference is measured in that scaling, sqrt(diag H) x, so that the
    # 1e-9 of test_hip_cholesky_per_phase_launches_agree_with_one_workgroup means the same for the badly scaled systems as for the others
    if 1 in by_batch and 49 in by_batch:
        diff = float(np.abs(d * (by_batch[1] - by_batch[49])).max() / np.abs(d * by_batch[1]).max())
        print("    batch 1 vs batch 49 (two plans): %.3e" % diff)
        assert diff < 1e-9, (kind, nfree, diff)
    print("    worst residual ratio: %.3f" % worst)
    return worst


def batches_for(nfree):
    return (1, 3, 49) if nfree <= 91 else (1, 3)    # 49 windows of up to 91 free key frames: 117 MB of systems


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nfree", SIZES)
def test_hip_reduced_solve_matches_longdouble(hip_lib, nfree, kind):
    check_solve(hip_lib, kind, nfree, batches_for(nfree))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nfree", [1, 2, 3, 5, 6, 11, 16])
def test_emu_reduced_solve_matches_longdouble(emu_lib, nfree, kind):
    """the emulated build takes the same plans as the product (the plan function is host code); its matrix instruction is plain C.
    (49 windows at two sizes only: the emulator runs a 512-thread workgroup per window as fibers)"""
    check_solve(emu_lib, kind, nfree, (1, 3, 49) if nfree in (5, 11) else (1, 3), tag="emu")


def test_emu_reduced_solve_lds_limit_pair():
    """WG_CHOL_LDS_MAX_LD=30 + LM_CHOL_SPLIT_MAX_BATCH=0 (the build of test_emu_lba_optimize_global_memory_panel): 5 free key frames are the
    last size with the panel in LDS, 6 the first with the panel in global memory — the 176 / 177 pair of the product at a size the emulator runs"""
    import build_emu
    lib = ctypes.CDLL(build_emu.build(defines=("WG_CHOL_LDS_MAX_LD=30", "LM_CHOL_SPLIT_MAX_BATCH=0"), tag="cholext"))
    for nfree, want in ((5, WG_NB16), (6, WG_NB16_GLOBAL)):
        for kind in KINDS:
            check_solve(lib, kind, nfree, (1, 3, 49), plan_of=lambda batch, nf: want, tag="emu cholext")


# ---- the failure flag -------------------------------------------------------------------------------------------------------------------------
FAIL_CASES = [(3, 16, PER_PANEL), (3, 90, PER_PANEL), (3, 120, WG_NB16), (3, 177, WG_NB16_GLOBAL), (49, 16, WG_NB16), (49, 60, WG_NB32)]


def check_failure_flag(lib, batch, nfree, want, bad=1):
    """One window of the batch is A - (lambda_min + 1) I: indefinite, finite.  It reports ok = 0 (what the LM loop turns into a rejected trial);
    every other window returns the bits it returns when a good window stands in its place."""
    plan = lm_plan(lib, batch, nfree, 1, 0, nfree)
    print("failure flag: nfree=%d batch=%d: plan %d (%s)" % (nfree, batch, plan["chol"], PLAN_NAMES[plan["chol"]]))
    assert plan["chol"] == want, "this case no longer takes plan '%s' but '%s'" % (PLAN_NAMES[want], PLAN_NAMES[plan["chol"]])
    ms = ragged(nfree, batch)
    refs = [reference("gram", nfree, m) for m in ms]
    mats, rhs = [r[0] for r in refs], [r[1] for r in refs]
    good, ok_good = solve_reduced(lib, mats, rhs, nfree)
    assert (ok_good == 1).all()
    A = mats[bad]
    Abad = A - (np.linalg.eigvalsh(A)[0] + 1.0) * np.eye(len(A))
    assert np.isfinite(Abad).all() and np.linalg.eigvalsh(Abad)[0] < -0.5
    got, ok = solve_reduced(lib, mats[:bad] + [Abad] + mats[bad + 1:], rhs, nfree)
    assert ok[bad] == 0 and (np.delete(ok, bad) == 1).all(), ok
    for i in range(batch):
        if i != bad:
            assert np.array_equal(got[i], good[i]), i


@pytest.mark.gpu
@pytest.mark.parametrize("batch,nfree,want", FAIL_CASES)
def test_hip_reduced_solve_failure_flag(hip_lib, batch, nfree, want):
    check_failure_flag(hip_lib, batch, nfree, want)
    if batch == 49:
        check_failure_flag(hip_lib, batch, nfree, want, bad=0)     # the largest window of the batch


@pytest.mark.parametrize("batch,nfree,want", [(3, 6, PER_PANEL), (3, 16, PER_PANEL), (49, 6, WG_NB16)])
def test_emu_reduced_solve_failure_flag(emu_lib, batch, nfree, want):
    check_failure_flag(emu_lib, batch, nfree, want)


def test_emu_reduced_solve_failure_flag_forced_plans():
    """the one-workgroup plans the emulator cannot reach at its sizes, under the forced-path builds the LM tests already use"""
    import build_emu
    for defines, tag, want in ((("WG_CHOL_LDS_MAX_LD=30", "LM_CHOL_SPLIT_MAX_BATCH=0"), "cholext", WG_NB16_GLOBAL),
                               (("WG_CHOL_NB32_MIN_LD=0", "LM_CHOL_SPLIT_MAX_BATCH=0"), "cholnb32mono", WG_NB32)):
        lib = ctypes.CDLL(build_emu.build(defines=defines, tag=tag))
        check_failure_flag(lib, 3, 11, want)
