"""Map-point refresh (orbm_refresh_map_points) against a numpy restatement of the two reference functions it replaces:
MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:372-460) and MapPoint::UpdateNormalAndDepth (MapPoint.cc:485-558).

The restatement: pairwise Hamming distances from np.unpackbits, median = np.sort(row)[int(0.5*(N-1))], winner = np.argmin (the first
minimum); the normal with the cv::Mat arithmetic of tests/cpp/mock_orbslam3/opencv2/core/core.hpp (`-` / `+` in float, cv::norm = sqrt of the
double dot product summed from 0, Mat / scalar = the scalar as a float and one float division per element, summed in record order).
Every output is compared bit for bit (NaN fields by class).  backend "emu": the product kernels compiled against tests/emu; "hip": the real
library on an MI355X."""
import ctypes

import numpy as np
import pytest

import orbhip
from devarrays import BACKENDS, bits, lib, to_dev, to_dev_plain, to_host  # noqa: F401
from orbhip._lib import ORB_E_CAPACITY, ORB_E_INVALID, OrbHipError, ptr
from orbhip.matcher import (KEYFRAME_CENTER_DTYPE, MAP_POINT_DTYPE, MP_BAD, MP_VALID, OBS_KF_BAD, OBS_RIGHT, OBSERVATION_DTYPE, PROJ_LOCAL_MAP,
                            QUERY_DTYPE, REFRESH_BAD_RECORD, REFRESH_DESCRIPTOR, REFRESH_MAX_OBS, REFRESH_NORMAL_DEPTH, REFRESH_OVERFLOW,
                            REFRESH_POINT_DTYPE, REFRESHED_DESCRIPTOR, REFRESHED_NORMAL_DEPTH, TRACK_DTYPE, flatten_observations)
from test_map_projection import CAM, LSF, MB, MBF, SF, make_frame, ref_frame

f32, f64 = np.float32, np.float64
BOTH = REFRESH_DESCRIPTOR | REFRESH_NORMAL_DEPTH
EPS = 2.0 ** -24
SENTINEL = 77


# ------------------------------------------------------------------------------------------------ restatement of the reference functions
def distances(desc):
    """all pairwise Hamming distances of desc [N, 32] uint8 -> int [N, N] (Distances[i][i] = 0)"""
    b = np.unpackbits(desc, axis=1).astype(np.int32)
    return b @ (1 - b).T + (1 - b) @ b.T


def row_medians(desc, upper=False):
    D = np.sort(distances(desc), axis=1)
    N = len(desc)
    return D[:, N // 2 if upper else int(0.5 * (N - 1))]


def distinctive(desc):
    """MapPoint.cc:414-452: the first row with the least (lower) median"""
    return int(np.argmin(row_medians(desc)))


def norm3(d):
    """cv::norm of a float 3-vector: sqrt of the double dot product summed from 0 (a double)"""
    s = f64(0)
    for k in range(3):
        s = s + f64(d[k]) * f64(d[k])
    return np.sqrt(s)


def normal_and_depth(pos, centers, o_ref, sf_level, sf_last):
    """MapPoint.cc:508-556 for the record centres in order -> (normal f32[3], min_distance, max_distance)"""
    with np.errstate(all="ignore"):
        normal = np.zeros(3, f32)
        for Ow in centers:
            d = pos - Ow                              # float
            normal = normal + d / f32(norm3(d))       # Mat / double: the scalar as a float, float division
        normal = normal / f32(len(centers))
        dist = f32(norm3(pos - o_ref))
        mx = dist * f32(sf_level)
        mn = mx / f32(sf_last)
    return normal.astype(f32), f32(mn), f32(mx)


def normal_and_depth_f64(pos, centers, o_ref, sf_level, sf_last):
    """the same formulas evaluated in float64 throughout, from the same float inputs (sanity guard, not the yardstick)"""
    with np.errstate(all="ignore"):
        d = pos.astype(f64)[None, :] - np.asarray(centers, f64)
        normal = (d / np.linalg.norm(d, axis=1)[:, None]).sum(0) / len(centers)
        mx = np.linalg.norm(pos.astype(f64) - o_ref.astype(f64)) * f64(sf_level)
    return normal, mx / f64(sf_last), mx


class Scene:
    """the device-resident map of one call as host arrays"""

    def __init__(self, mp, mp_desc, points, ref, kf, kf_desc, sf=SF):
        self.mp, self.mp_desc, self.points, self.ref, self.kf, self.kf_desc, self.sf = mp, mp_desc, points, ref, kf, kf_desc, np.asarray(sf, f32)

    def flat(self):
        return flatten_observations(self.points)


def expected(S, what, sel=None, guard=None):
    """the restatement over the selected points -> (mp after, mp_desc after, best_obs, status); unselected entries hold SENTINEL"""
    mp, mp_desc = S.mp.copy(), S.mp_desc.copy()
    n = len(mp)
    best, status = np.full(n, SENTINEL, np.int32), np.full(n, SENTINEL, np.int32)
    nl = len(S.sf)
    for p in (range(n) if sel is None else sel):
        if p < 0 or p >= n:
            continue
        best[p], status[p] = -1, 0
        ob = np.asarray(S.points[p], np.int64).reshape(-1, 3)
        fl = int(S.mp[p]["flags"])
        if not (fl & MP_VALID) or (fl & MP_BAD) or len(ob) == 0:
            continue
        in_range = (ob[:, 0] >= 0) & (ob[:, 0] < len(S.kf)) & (ob[:, 1] >= 0) & (ob[:, 1] < len(S.kf_desc))
        usable = in_range & ((ob[:, 2] & OBS_KF_BAD) == 0)
        st = 0 if in_range.all() else REFRESH_BAD_RECORD
        if usable.sum() > REFRESH_MAX_OBS:
            status[p] = st | REFRESH_OVERFLOW
            continue
        if (what & REFRESH_DESCRIPTOR) and usable.any():
            idx = np.nonzero(usable)[0]
            w = idx[distinctive(S.kf_desc[ob[idx, 1]])]
            best[p] = w
            row = int(S.mp[p]["desc_row"])
            if 0 <= row < len(mp_desc):
                mp_desc[row] = S.kf_desc[ob[w, 1]]
            st |= REFRESHED_DESCRIPTOR
        if (what & REFRESH_NORMAL_DEPTH) and in_range.any():
            rk, lv = int(S.ref[p]["ref_kf"]), int(S.ref[p]["level"])
            if 0 <= rk < len(S.kf) and 0 <= lv < nl:
                centers = [S.kf[k]["right" if f & OBS_RIGHT else "left"] for k, _, f in ob[in_range]]
                pos = np.array(S.mp[p]["pos"], f32)
                args = (pos, centers, S.kf[rk]["left"], S.sf[lv], S.sf[nl - 1])
                mp[p]["normal"], mp[p]["min_distance"], mp[p]["max_distance"] = normal_and_depth(*args)
                if guard is not None:
                    guard.append((p, len(centers)) + normal_and_depth_f64(*args))
                st |= REFRESHED_NORMAL_DEPTH
            else:
                st |= REFRESH_BAD_RECORD
        status[p] = st
    return mp, mp_desc, best, status


# ------------------------------------------------------------------------------------------------ scenes
def keyframes(rng, n_kf=48):
    """key frames on a circle of radius 3 m, the right camera 0.11 m along the tangent"""
    kf = np.zeros(n_kf, KEYFRAME_CENTER_DTYPE)
    a = np.linspace(0, 2 * np.pi, n_kf, endpoint=False)
    kf["left"] = np.stack([3 * np.cos(a), 0.2 * rng.normal(size=n_kf), 3 * np.sin(a)], 1).astype(f32)
    kf["right"] = (kf["left"] + 0.11 * np.stack([-np.sin(a), 0 * a, np.cos(a)], 1)).astype(f32)
    return kf


def make_scene(rng, Ns, n_kf=48, sf=SF, flip=0.08, right=0.3):
    """One point per entry of Ns (its observation count): a random 32-byte base, every bit of every observation flipped with probability
    `flip`; positions 2-10 m from a key frame; the descriptor rows of both slabs permuted."""
    n, total = len(Ns), int(np.sum(Ns))
    kf = keyframes(rng, n_kf)
    rows = rng.permutation(total + 5)
    kf_desc = rng.integers(0, 256, (total + 5, 32), dtype=np.uint8)
    mp = np.zeros(n, MAP_POINT_DTYPE)
    ref = np.zeros(n, REFRESH_POINT_DTYPE)
    points, r0 = [], 0
    for p, N in enumerate(Ns):
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        d = np.packbits(np.unpackbits(base)[None, :] ^ (rng.random((N, 256)) < flip), axis=1)
        kf_desc[rows[r0:r0 + N]] = d
        kfs = rng.integers(0, n_kf, N)
        fl = np.where(rng.random(N) < right, OBS_RIGHT, 0)
        points.append([(int(kfs[i]), int(rows[r0 + i]), int(fl[i])) for i in range(N)])
        r0 += N
        near = kf["left"][kfs[0] if N else 0].astype(f64)
        v = rng.normal(size=3)
        mp[p]["pos"] = (near + v / np.linalg.norm(v) * rng.uniform(2, 10)).astype(f32)
        ref[p] = (kfs[rng.integers(0, N)] if N else 0, rng.integers(0, len(sf)))
    mp["normal"] = rng.normal(size=(n, 3)).astype(f32)          # stale values the call has to replace (or keep)
    mp["min_distance"], mp["max_distance"] = rng.uniform(0.1, 1, n), rng.uniform(5, 50, n)
    mp["angle"], mp["octave"] = rng.uniform(0, 360, n), rng.integers(0, len(sf), n)
    mp["desc_row"] = rng.permutation(n + 3)[:n]
    mp["flags"] = MP_VALID
    return Scene(mp, rng.integers(0, 256, (n + 3, 32), dtype=np.uint8), points, ref, kf, kf_desc, sf)


def population(rng, n):
    return make_scene(rng, rng.integers(1, 41, n))


# ------------------------------------------------------------------------------------------------ running the library
def run(lib, backend, S, what, sel=None):
    """-> (mp after, mp_desc after, best_obs, status) as host arrays; best_obs / status start at SENTINEL"""
    m = orbhip.ORBmatcher(lib=lib)
    start, obs = S.flat()
    d_mp, d_desc = to_dev(S.mp.copy(), backend), to_dev_plain(S.mp_desc.copy(), backend)
    out = dict(best_obs=to_dev_plain(np.full(len(S.mp), SENTINEL, np.int32), backend), status=to_dev_plain(np.full(len(S.mp), SENTINEL, np.int32), backend))
    d_sel = None if sel is None else to_dev_plain(np.asarray(sel, np.int32), backend)
    res = m.RefreshMapPoints(d_mp, d_desc, to_dev_plain(start, backend), to_dev(obs, backend), to_dev(S.ref, backend), to_dev(S.kf, backend),
                             to_dev_plain(S.kf_desc, backend), m.RefreshParams(S.sf, what), sel=d_sel, out=out)
    if backend == "hip":
        import torch
        torch.cuda.synchronize()
    assert res is out
    return to_host(d_mp).reshape(-1).view(MAP_POINT_DTYPE), to_host(d_desc), to_host(out["best_obs"]), to_host(out["status"])


def check(lib, backend, S, what=BOTH, sel=None, guard=None):
    mp_e, desc_e, best_e, st_e = expected(S, what, sel, guard)
    mp, desc, best, st = run(lib, backend, S, what, sel)
    assert np.array_equal(best, best_e), np.nonzero(best != best_e)[0][:10]
    assert np.array_equal(st, st_e), np.nonzero(st != st_e)[0][:10]
    assert np.array_equal(desc, desc_e), np.nonzero((desc != desc_e).any(1))[0][:10]
    assert np.array_equal(bits(mp), bits(mp_e)), np.nonzero((bits(mp).reshape(len(mp), -1) != bits(mp_e).reshape(len(mp), -1)).any(1))[0][:10]
    return mp, desc, best, st


def check_guard(mp, guard):
    """case 2's independent guard: |normal - float64 normal| <= (n + 10) 2^-24 per component, the distances within 4 * 2^-24 relative"""
    assert len(guard) > 0
    for p, n, normal, mn, mx in guard:
        if not np.isfinite(normal).all():
            continue
        assert np.all(np.abs(mp[p]["normal"].astype(f64) - normal) <= (n + 10) * EPS), (p, n)
        assert abs(f64(mp[p]["max_distance"]) - mx) <= 4 * EPS * mx and abs(f64(mp[p]["min_distance"]) - mn) <= 4 * EPS * mn, p


# ------------------------------------------------------------------------------------------------ case 1 + 2: the random population
def test_generator_covers_the_deciding_classes():
    """conditions on the inputs of test_population: ties at the least median, winners other than row 0, lower != upper median choices"""
    S = population(np.random.default_rng(101), 600)
    ties = nonzero = upper = 0
    for obs in S.points:
        d = S.kf_desc[[r for _, r, _ in obs]]
        med = row_medians(d)
        ties += int((med == med.min()).sum() > 1)
        nonzero += int(np.argmin(med) != 0)
        upper += int(np.argmin(row_medians(d, upper=True)) != np.argmin(med))
    assert ties >= 60 and nonzero >= 300 and upper >= 20, (ties, nonzero, upper)


@pytest.mark.parametrize("backend", BACKENDS)
def test_population(lib, backend):
    """600 points (emu) / 6000 points (hip), N uniform in 1..40: descriptor choice, slab bytes, normal, min / max distance, bit exact"""
    S = population(np.random.default_rng(101), 600 if backend == "emu" else 6000)
    guard = []
    mp, _, best, st = check(lib, backend, S, guard=guard)
    assert (st == (REFRESHED_DESCRIPTOR | REFRESHED_NORMAL_DEPTH)).all() and (best >= 0).all()
    assert not np.array_equal(mp["normal"], S.mp["normal"])
    check_guard(mp, guard)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("nlevels", [8, 1])
def test_levels_and_camera_centres(lib, backend, nlevels):
    """every level 0..nlevels-1 as the reference octave, left and right centres, nlevels 8 and 1; one point exactly at a camera centre"""
    rng = np.random.default_rng(102 + nlevels)
    S = make_scene(rng, rng.integers(1, 41, 64), sf=SF[:nlevels], right=0.5)
    S.ref["level"] = np.arange(64) % nlevels
    S.mp[5]["pos"] = S.kf[S.points[5][0][0]]["right" if S.points[5][0][2] & OBS_RIGHT else "left"]   # 0/0: NaN normal
    S.mp[6]["pos"] = S.kf[S.ref[6]["ref_kf"]]["left"]                                                # dist = 0
    flags = np.array([f for obs in S.points for _, _, f in obs])
    assert (flags & OBS_RIGHT).any() and not (flags & OBS_RIGHT).all()
    guard = []
    mp, _, _, _ = check(lib, backend, S, guard=guard)
    assert np.isnan(mp[5]["normal"]).all() and set(S.ref["level"]) == set(range(nlevels))
    check_guard(mp, guard)


# ------------------------------------------------------------------------------------------------ case 1: the named edge cases
def special_scene(rng):
    """0: N = 1, 1: N = 2, 2: all descriptors equal, 3-5: N = 64 / 65 / 129, 6: bad key frames among the records, 7: all key frames bad,
    8: no observations, 9: ORBM_MP_BAD, 10: not ORBM_MP_VALID, 11 / 12: desc_row out of range, 13: out-of-range records, 14: bad ref_kf,
    15: bad level, 16: every record out of range"""
    S = make_scene(rng, [1, 2, 9, 64, 65, 129, 30, 6, 0, 12, 12, 10, 10, 14, 8, 8, 3])
    same = S.kf_desc[S.points[2][0][1]].copy()
    for _, r, _ in S.points[2]:
        S.kf_desc[r] = same
    # bad key frames: the winner of the remaining rows changes and best_obs counts the skipped records
    S.points[6] = [(k, r, f | (OBS_KF_BAD if i % 3 == 0 else 0)) for i, (k, r, f) in enumerate(S.points[6])]
    S.points[7] = [(k, r, f | OBS_KF_BAD) for k, r, f in S.points[7]]
    S.mp[9]["flags"] |= MP_BAD
    S.mp[10]["flags"] = 0
    S.mp[11]["desc_row"], S.mp[12]["desc_row"] = -1, len(S.mp_desc)
    P = S.points[13]
    P[0] = (-1, P[0][1], P[0][2])
    P[3] = (len(S.kf), P[3][1], P[3][2])
    P[5] = (P[5][0], -1, P[5][2])
    P[9] = (P[9][0], len(S.kf_desc), P[9][2])
    S.ref[14]["ref_kf"] = len(S.kf)
    S.ref[15]["level"] = len(S.sf)
    S.points[16] = [(-5, r, f) for _, r, f in S.points[16]]
    return S


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("what", [BOTH, REFRESH_DESCRIPTOR, REFRESH_NORMAL_DEPTH])
def test_edge_cases(lib, backend, what):
    """the named cases, for both halves together and for each alone (check() compares every byte of the records and of the slab, so the half
    that was not asked for, the untouched rows and the untouched points are byte-identical to before)"""
    S = special_scene(np.random.default_rng(103))
    mp, desc, best, st = check(lib, backend, S, what)
    D, Nn = what & REFRESH_DESCRIPTOR, what & REFRESH_NORMAL_DEPTH
    if D:
        assert best[0] == 0 and best[1] == 0 and best[2] == 0                       # N = 1, N = 2 and all-equal choose the first
        assert best[6] % 3 != 0 and best[7] == -1 and best[11] >= 0 and best[12] >= 0
        assert np.array_equal(desc, expected(S, what)[1]) and not np.array_equal(desc[S.mp[6]["desc_row"]], S.mp_desc[S.mp[6]["desc_row"]])
    else:
        assert (best == -1).all() and np.array_equal(desc, S.mp_desc)
    if Nn:
        assert st[7] == REFRESHED_NORMAL_DEPTH                                       # bad key frames still count for the normal
        assert not np.array_equal(mp[7]["normal"], S.mp[7]["normal"])
        assert st[14] & REFRESH_BAD_RECORD and st[15] & REFRESH_BAD_RECORD and not (st[14] | st[15]) & REFRESHED_NORMAL_DEPTH
    else:
        for name in ("normal", "min_distance", "max_distance"):
            assert np.array_equal(mp[name], S.mp[name])
    for p in (8, 9, 10):
        assert best[p] == -1 and st[p] == 0 and mp[p] == S.mp[p]
    assert st[13] & REFRESH_BAD_RECORD and st[16] == REFRESH_BAD_RECORD and best[16] == -1 and mp[16] == S.mp[16]
    for name in ("pos", "angle", "octave", "desc_row", "flags"):
        assert np.array_equal(mp[name], S.mp[name])


@pytest.mark.parametrize("backend", BACKENDS)
def test_cap_and_overflow(lib, backend):
    """one point at ORBM_REFRESH_MAX_OBS (refreshed), one at MAX_OBS + 1 (flagged, untouched), one with more records but MAX_OBS usable"""
    rng = np.random.default_rng(104)
    S = make_scene(rng, [REFRESH_MAX_OBS, REFRESH_MAX_OBS + 1, REFRESH_MAX_OBS + 6, 5])
    S.points[2] = [(k, r, f | (OBS_KF_BAD if i % 200 == 3 else 0)) for i, (k, r, f) in enumerate(S.points[2])]
    assert sum(1 for _, _, f in S.points[2] if not f & OBS_KF_BAD) == REFRESH_MAX_OBS
    mp, desc, best, st = check(lib, backend, S)
    full = REFRESHED_DESCRIPTOR | REFRESHED_NORMAL_DEPTH
    assert list(st) == [full, REFRESH_OVERFLOW, full, full] and best[1] == -1 and best[0] >= 0 and best[2] >= 0
    assert mp[1] == S.mp[1] and np.array_equal(desc[S.mp[1]["desc_row"]], S.mp_desc[S.mp[1]["desc_row"]])
    m = orbhip.ORBmatcher(lib=lib)
    with pytest.raises(OrbHipError) as e:
        m.check_refresh_overflow(dict(status=st))
    assert e.value.code == ORB_E_CAPACITY
    m.check_refresh_overflow(dict(status=st), sel=np.array([0, 2, 3], np.int32))


@pytest.mark.parametrize("backend", BACKENDS)
def test_selection(lib, backend):
    """d_sel: a strict subset in non-ascending order (plus out-of-range entries, which are skipped); unselected points byte-identical"""
    S = make_scene(np.random.default_rng(105), [3, 70, 12, 1, 40, 66, 9, 2, 30, 17])
    sel = [8, 1, 6, 2, -1, 5, len(S.mp)]
    mp, desc, best, st = check(lib, backend, S, sel=sel)
    for p in (0, 3, 4, 7, 9):
        assert best[p] == SENTINEL and st[p] == SENTINEL and mp[p] == S.mp[p]
        assert np.array_equal(desc[S.mp[p]["desc_row"]], S.mp_desc[S.mp[p]["desc_row"]])
    assert all(st[p] == (REFRESHED_DESCRIPTOR | REFRESHED_NORMAL_DEPTH) for p in (8, 1, 6, 2, 5))


# ------------------------------------------------------------------------------------------------ case 3: order sensitivity
@pytest.mark.parametrize("backend", BACKENDS)
def test_record_order_is_semantic(lib, backend):
    rng = np.random.default_rng(106)
    S = make_scene(rng, rng.integers(2, 41, 200))
    T = Scene(S.mp, S.mp_desc, [[obs[i] for i in rng.permutation(len(obs))] for obs in S.points], S.ref, S.kf, S.kf_desc, S.sf)
    mpS, _, bestS, _ = check(lib, backend, S)
    mpT, _, bestT, _ = check(lib, backend, T)
    # not vacuous: a tie that the order decides (another descriptor row wins), and a float sum that depends on the order
    rowS = np.array([S.points[p][bestS[p]][1] for p in range(200)])
    rowT = np.array([T.points[p][bestT[p]][1] for p in range(200)])
    assert (rowS != rowT).sum() >= 5
    assert (mpS["normal"].view(np.uint32) != mpT["normal"].view(np.uint32)).any(1).sum() >= 5
    assert np.array_equal(mpS["max_distance"], mpT["max_distance"])


# ------------------------------------------------------------------------------------------------ case 4: chaining into the projection
def chain_scene(rng, n):
    """points in front of a camera at the origin (the key frames on their circle around it), a spread of depths"""
    S = make_scene(rng, rng.integers(1, 41, n))
    z = rng.uniform(4, 12, n)
    S.mp["pos"] = np.stack([rng.uniform(-0.7, 0.7, n) * z, rng.uniform(-0.45, 0.45, n) * z, z], 1).astype(f32)
    track = np.zeros((1, n), TRACK_DTYPE)
    return S, make_frame(np.eye(3, dtype=f32), np.zeros(3, f32)), track


def expected_chain(S, F, track, cap_q):
    mp_e, desc_e, best_e, st_e = expected(S, BOTH)
    q, qd, src, req, nin, tr = ref_frame(mp_e, len(mp_e), desc_e, F, track[0], PROJ_LOCAL_MAP, 3.0)
    return mp_e, desc_e, best_e, st_e, q, qd, src, req, nin, tr


def compare_chain(exp, d_mp, d_desc, ref_out, proj, cap_q):
    mp_e, desc_e, best_e, st_e, q, qd, src, req, nin, tr = exp
    assert np.array_equal(to_host(ref_out["best_obs"]), best_e) and np.array_equal(to_host(ref_out["status"]), st_e)
    assert np.array_equal(bits(to_host(d_mp).reshape(-1).view(MAP_POINT_DTYPE)), bits(mp_e)) and np.array_equal(to_host(d_desc), desc_e)
    assert req <= cap_q and nin > 50, (req, nin)
    assert (int(to_host(proj["n_required"])[0]), int(to_host(proj["n_in_view"])[0]), int(to_host(proj["nq"])[0])) == (req, nin, req)
    Q = to_host(proj["queries"]).reshape(1, cap_q, -1).view(QUERY_DTYPE)[0, :, 0]
    assert np.array_equal(bits(Q[:req]), bits(q)) and np.array_equal(to_host(proj["qdesc"])[0, :req], qd)
    assert np.array_equal(to_host(proj["q_src"])[0, :req], src)
    assert np.array_equal(bits(to_host(proj["track"]).reshape(-1).view(TRACK_DTYPE)), bits(tr))


def chain_calls(m, D, prm_r, prm_p, n, ref_out=None, proj=None):
    ref_out = m.RefreshMapPoints(D["mp"], D["mp_desc"], D["start"], D["obs"], D["ref"], D["kf"], D["kf_desc"], prm_r, out=ref_out)
    proj = m.ProjectMapPoints(D["mp"], D["nmp"], D["mp_desc"], D["frames"], prm_p, n, track=D["track"], out=proj)
    return ref_out, proj


def chain_buffers(S, F, track, backend):
    start, obs = S.flat()
    n = len(S.mp)
    return dict(mp=to_dev(S.mp.copy().reshape(1, n), backend), mp_desc=to_dev_plain(S.mp_desc.copy(), backend), start=to_dev_plain(start, backend),
                obs=to_dev(obs, backend), ref=to_dev(S.ref, backend), kf=to_dev(S.kf, backend), kf_desc=to_dev_plain(S.kf_desc, backend),
                nmp=to_dev_plain(np.array([n], np.int32), backend), frames=to_dev(np.array([F]), backend),
                track=track.copy() if backend == "emu" else to_dev(track, backend))


def chain_params(m, S):
    return m.RefreshParams(S.sf), m.ProjectParams(PROJ_LOCAL_MAP, CAM, SF, LSF, 3.0, mbf=MBF, mb=MB)


@pytest.mark.parametrize("backend", BACKENDS)
def test_refresh_then_project(lib, backend):
    """refresh, then ProjectMapPoints (LOCAL_MAP) on the same buffers and stream with no host read in between == the restatement of both"""
    n = 400 if backend == "emu" else 3000
    S, F, track = chain_scene(np.random.default_rng(107), n)
    m = orbhip.ORBmatcher(0.8, True, lib=lib)
    D = chain_buffers(S, F, track, backend)
    ref_out, proj = chain_calls(m, D, *chain_params(m, S), n)
    compare_chain(expected_chain(S, F, track, n), D["mp"], D["mp_desc"], ref_out, proj, n)


@pytest.mark.gpu
def test_refresh_then_project_graph_replay_hip(hip_lib):
    """both launches captured into one graph, replayed twice with the positions changed in between (the points the optimiser moved)"""
    import torch
    rng = np.random.default_rng(108)
    n = 3000
    S, F, track = chain_scene(rng, n)
    m = orbhip.ORBmatcher(0.8, True, lib=hip_lib)
    D = chain_buffers(S, F, track, "hip")
    prm_r, prm_p = chain_params(m, S)
    mp0, desc0, track0 = D["mp"].clone(), D["mp_desc"].clone(), D["track"].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ref_out, proj = chain_calls(m, D, prm_r, prm_p, n)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    compare_chain(expected_chain(S, F, track, n), D["mp"], D["mp_desc"], ref_out, proj, n)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain_calls(m, D, prm_r, prm_p, n, ref_out, proj)
    for it in range(2):
        S.mp["pos"] = (S.mp["pos"] + rng.normal(0, 0.05, (n, 3))).astype(f32)
        D["mp"].copy_(to_dev(S.mp.reshape(1, n), "hip"))
        D["mp_desc"].copy_(desc0)
        D["track"].copy_(track0)
        for v in list(ref_out.values()) + [proj[k] for k in ("queries", "qdesc", "nq", "q_src", "n_required", "n_in_view")]:
            v.fill_(90)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        compare_chain(expected_chain(S, F, track, n), D["mp"], D["mp_desc"], ref_out, proj, n)
    assert not torch.equal(mp0, D["mp"])


# ------------------------------------------------------------------------------------------------ case 5: errors
@pytest.mark.parametrize("backend", BACKENDS)
def test_argument_errors(lib, backend):
    S = make_scene(np.random.default_rng(109), [4, 7, 2])
    m = orbhip.ORBmatcher(lib=lib)
    start, obs = S.flat()
    dv, dp = (lambda a: to_dev(a, backend)), (lambda a: to_dev_plain(a, backend))
    good = dict(mp=dv(S.mp.copy()), mp_desc=dp(S.mp_desc.copy()), obs_start=dp(start), obs=dv(obs), ref=dv(S.ref), kf=dv(S.kf),
                kf_desc=dp(S.kf_desc))
    out = dict(best_obs=dp(np.full(3, SENTINEL, np.int32)), status=dp(np.full(3, SENTINEL, np.int32)))

    def call(prm=None, sel=None, **kw):
        a = dict(good, **kw)
        return m.RefreshMapPoints(a["mp"], a["mp_desc"], a["obs_start"], a["obs"], a["ref"], a["kf"], a["kf_desc"],
                                  prm if prm is not None else m.RefreshParams(S.sf), sel=sel, out=kw.get("out", out))

    def invalid(**kw):
        with pytest.raises(OrbHipError) as e:
            call(**kw)
        assert e.value.code == ORB_E_INVALID, kw.keys()

    for what in (0, 4, 7, 1 << 31):
        invalid(prm=m.RefreshParams(S.sf, what))
    for nl in (0, 17, -1):
        p = m.RefreshParams(S.sf)
        p.nlevels = nl
        invalid(prm=p)
    L = m._L
    args = [good["mp"], 3, good["mp_desc"], len(S.mp_desc), None, 0, good["obs_start"], good["obs"], good["ref"], good["kf"], len(S.kf),
            good["kf_desc"], len(S.kf_desc), None, out["best_obs"], out["status"]]
    names = ["mp", None, "mp_desc", None, None, None, "obs_start", "obs", "ref", "kf", None, "kf_desc", None, "params", "best_obs", "status"]
    prm = m.RefreshParams(S.sf)

    def raw(null=None, over=()):
        """the C entry point with one argument nulled / some positions replaced"""
        a = list(args)
        for k, v in dict(over).items():
            a[k] = v
        c = [ctypes.byref(prm) if nm == "params" else (x if isinstance(x, int) else ptr(x)) for nm, x in zip(names, a)]
        if null is not None:
            c[names.index(null)] = None
        return L.orbm_refresh_map_points(*c, None)
    assert raw() == 0
    for nm in ("mp", "mp_desc", "obs_start", "obs", "ref", "kf", "kf_desc", "params", "best_obs", "status"):
        assert raw(null=nm) == ORB_E_INVALID, nm
    for pos in (1, 3, 10, 12):                       # n_mp, n_desc_rows, n_kf, n_kf_desc_rows
        assert raw(over={pos: -1}) == ORB_E_INVALID, pos
    sel = dp(np.array([1], np.int32))
    assert raw(over={4: sel, 5: -1}) == ORB_E_INVALID   # negative n_sel with a selection
    # successful no-ops: n_sel == 0 with a selection, n_mp == 0
    assert raw(over={4: sel, 5: 0}) == 0 and raw(over={1: 0}) == 0
    call(sel=dp(np.zeros(0, np.int32)))
    if backend == "hip":
        import torch
        torch.cuda.synchronize()
    after = [to_host(out["best_obs"]), to_host(out["status"]), to_host(good["mp"]), to_host(good["mp_desc"])]
    # (raw() without a selection above refreshed all three points once: compare against the state after it)
    mp_e, desc_e, best_e, st_e = expected(S, BOTH)
    assert np.array_equal(after[0], best_e) and np.array_equal(after[1], st_e) and np.array_equal(after[3], desc_e)
    assert np.array_equal(bits(after[2].reshape(-1).view(MAP_POINT_DTYPE)), bits(mp_e))
    # a misaligned descriptor slab is refused
    if backend == "emu":
        buf = np.zeros(len(S.kf_desc) * 32 + 16, np.uint8)
        off = (-buf.ctypes.data) % 16 + 4
        invalid(kf_desc=buf[off:off + len(S.kf_desc) * 32].reshape(-1, 32))
    with pytest.raises(OrbHipError):
        call(obs_start=dp(start[:-1].copy()))


# ------------------------------------------------------------------------------------------------ case 7: the observation CSR
def test_flatten_observations():
    start, obs = flatten_observations([[(1, 2, 0), (3, 4, OBS_RIGHT)], [], [(5, 6, OBS_KF_BAD)]])
    assert list(start) == [0, 2, 2, 3] and obs.dtype == OBSERVATION_DTYPE
    assert [tuple(int(v) for v in o) for o in obs] == [(1, 2, 0), (3, 4, OBS_RIGHT), (5, 6, OBS_KF_BAD)]
