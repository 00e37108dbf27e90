"""Map-point projection (orbm_project_map_points) against a numpy restatement of the reference loops it replaces:
Frame::isInFrustum + Tracking::SearchLocalPoints + the query loop of SearchByProjection(Frame&, vector<MapPoint*>&, ...) (LOCAL_MAP),
the projection of SearchByProjection(Frame&, const Frame&, th, bMono) (LAST_FRAME) and of SearchByProjection(Frame&, KeyFrame*, ...) (RELOC).

The restatement follows the cv::Mat arithmetic of tests/cpp/mock_orbslam3/opencv2/core/core.hpp (R*X summed in double from 0 and rounded
once, `+ t` and Pinhole::project in float, cv::norm = float(sqrt(double dot)), PO.dot(Pn)/dist in double) and calls glibc's logf for
MapPoint::PredictScale.  Every output is compared bit for bit.  backend "emu": the product kernels compiled against tests/emu; "hip": the
real library on an MI355X."""
import ctypes
import math

import numpy as np
import pytest

import orbhip
from devarrays import bits, to_dev, to_dev_plain, to_host
from orbhip import KP_DTYPE
from orbhip._lib import ORB_E_CAPACITY, ORB_E_INVALID, OrbHipError
from orbhip.matcher import (MAP_POINT_DTYPE, MODE_BEST_ONLY, MODE_LOCAL_MAP, MP_BAD, MP_HAS_OBS, MP_SEEN, MP_VALID, PROJ_LAST_FRAME,
                            PROJ_LOCAL_MAP, PROJ_RELOC, PROJECT_FRAME_DTYPE, Q_HAS_OBS, Q_STEREO, Q_VALID, QUERY_DTYPE, TH_HIGH, TRACK_DTYPE)

f32, f64 = np.float32, np.float64
W, H = 752, 480
CAM = (f32(458.654), f32(457.296), f32(367.215), f32(248.375))
MBF, MB = f32(47.9), f32(0.11)
NLEVELS, SCALE = 8, f32(1.2)
SF = np.array([SCALE ** i for i in range(NLEVELS)], np.float32)   # mvScaleFactors as ORBextractor fills them (float products)
for _i in range(1, NLEVELS):
    SF[_i] = SF[_i - 1] * SCALE
LSF = f32(math.log(SCALE))   # mfLogScaleFactor = log(mfScaleFactor)
GRID = (0.0, 0.0, float(f32(64) / f32(W)), float(f32(48) / f32(H)))

_libm = ctypes.CDLL("libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def logf(x):
    return f32(_libm.logf(float(x)))


# ------------------------------------------------------------------------------------------------ restatement of the reference loops
def mat_rows(R, X):
    """cv::Mat R*X for a 3x3 float R (row-major [9]) and points X [n,3]: per row, double sum from 0 of the products, rounded once."""
    out = np.empty((len(X), 3), np.float32)
    for r in range(3):
        s = np.zeros(len(X), f64)
        for k in range(3):
            s = s + f64(R[3 * r + k]) * X[:, k].astype(f64)
        out[:, r] = s.astype(f32)
    return out


def dot3(A, B):
    s = np.zeros(len(A), f64)
    for k in range(3):
        s = s + A[:, k].astype(f64) * B[:, k].astype(f64)
    return s


def predict_scale(ratio, lsf=LSF, nlevels=NLEVELS):
    """MapPoint::PredictScale: int(ceil(std::log(float ratio) / mfLogScaleFactor)), clamped; x86 converts non-finite values to INT_MIN."""
    out = np.zeros(len(ratio), np.int32)
    cache = {}
    for j, r in enumerate(np.asarray(ratio, np.float32)):
        key = r.view(np.uint32).item()
        if key not in cache:
            c = np.ceil(logf(r) / f32(lsf))
            n = int(c) if np.isfinite(c) else -2 ** 31
            cache[key] = 0 if n < 0 else min(n, nlevels - 1)
        out[j] = cache[key]
    return out


def project(X, F, cam=CAM):
    """Pc = Rcw*X + tcw, uv = Pinhole::project(Pc), the bounds test (true = inside)"""
    fx, fy, cx, cy = cam
    R = F["Rcw"]
    Pc = mat_rows(R, X) + F["tcw"][None, :]
    with np.errstate(all="ignore"):
        u = fx * Pc[:, 0] / Pc[:, 2] + cx
        v = fy * Pc[:, 1] / Pc[:, 2] + cy
    b = F["bounds"]
    inside = ~((u < b[0]) | (u > b[1])) & ~((v < b[2]) | (v > b[3]))
    return Pc, u, v, inside


def ref_frame(mp, n, desc, F, track, mode, th, mono=True, view_cos_limit=f32(0.5), far=False, th_far=f32(0), cap_q=None, sf=SF,
              lsf=LSF, nlevels=NLEVELS):
    """One frame of the reference loops -> (queries QUERY_DTYPE[n_required], qdesc, q_src, n_required, n_in_view, track after)"""
    mp = mp[:n]
    X = np.ascontiguousarray(mp["pos"])
    fl = mp["flags"]
    valid, bad = (fl & MP_VALID) != 0, (fl & MP_BAD) != 0
    Pc, u, v, inside = project(X, F)
    zc = Pc[:, 2]
    th = f32(th)
    T = track[:n].copy() if track is not None else None
    with np.errstate(all="ignore"):
        PO = X - F["Ow"][None, :]
        dist = np.sqrt(dot3(PO, PO)).astype(f32)
        dist_ok = ~((dist < f32(0.8) * mp["min_distance"]) | (dist > f32(1.2) * mp["max_distance"]))
        ratio = mp["max_distance"] / dist
        if mode == PROJ_LOCAL_MAP:
            proc = valid & ((fl & (MP_SEEN | MP_BAD)) == 0)
            T["in_view"][proc] = 0
            T["proj_x"][proc] = -1
            T["proj_y"][proc] = -1
            invz = f32(1) / zc
            pc_dist = np.sqrt(dot3(Pc, Pc)).astype(f32)
            ok = proc & ~(zc < f32(0)) & inside
            T["proj_x"][ok] = u[ok]
            T["proj_y"][ok] = v[ok]
            ok &= dist_ok
            view_cos = (dot3(PO, np.ascontiguousarray(mp["normal"])) / dist.astype(f64)).astype(f32)
            ok &= ~(view_cos < f32(view_cos_limit))
            T["in_view"][ok] = 1
            T["proj_xr"][ok] = u[ok] - MBF * invz[ok]
            T["depth"][ok] = pc_dist[ok]
            T["level"][ok] = predict_scale(ratio[ok], lsf, nlevels)
            T["view_cos"][ok] = view_cos[ok]
            n_in_view = int(ok.sum())
            sel = valid & (T["in_view"] != 0) & ~(far & (T["depth"] > f32(th_far))) & ~bad
            L = T["level"][sel]
            r = np.where(T["view_cos"][sel].astype(f64) > 0.998, f32(2.5), f32(4.0)).astype(f32)
            if th != f32(1.0):
                r = r * th
            q = np.zeros(int(sel.sum()), QUERY_DTYPE)
            q["u"], q["v"], q["radius"], q["u_right"] = T["proj_x"][sel], T["proj_y"][sel], r * sf[L], T["proj_xr"][sel]
            q["min_level"], q["max_level"] = L - 1, L
            q["flags"] = Q_VALID | Q_STEREO | np.where(fl[sel] & MP_HAS_OBS, Q_HAS_OBS, 0)
            if n_in_view == 0:
                q, sel = q[:0], np.zeros_like(sel)
        elif mode == PROJ_LAST_FRAME:
            Ow = F["Ow"][None, :]
            tlc_z = mat_rows(F["Rlw"], Ow)[0, 2] + F["tlw"][2]
            fwd = bool(tlc_z > MB) and not mono
            bwd = bool(-tlc_z > MB) and not mono
            invzc = (1.0 / zc.astype(f64)).astype(f32)
            sel = valid & ~(invzc < 0) & inside
            o = mp["octave"][sel]
            q = np.zeros(int(sel.sum()), QUERY_DTYPE)
            q["u"], q["v"], q["radius"], q["u_right"], q["angle"] = u[sel], v[sel], th * sf[o], u[sel] - MBF * invzc[sel], mp["angle"][sel]
            q["min_level"] = o if fwd else (np.zeros_like(o) if bwd else o - 1)
            q["max_level"] = np.full_like(o, -1) if fwd else (o if bwd else o + 1)
            q["flags"] = Q_VALID | Q_STEREO | np.where(fl[sel] & MP_HAS_OBS, Q_HAS_OBS, 0)
            n_in_view = int(sel.sum())
        else:
            sel = valid & ~bad & inside & dist_ok
            L = predict_scale(ratio[sel], lsf, nlevels)
            q = np.zeros(int(sel.sum()), QUERY_DTYPE)
            q["u"], q["v"], q["radius"], q["angle"] = u[sel], v[sel], th * sf[L], mp["angle"][sel]
            q["min_level"], q["max_level"] = L - 1, L + 1
            q["flags"] = Q_VALID | Q_HAS_OBS
            n_in_view = int(sel.sum())
    src = np.nonzero(sel)[0].astype(np.int32)
    rows = mp["desc_row"][src]
    qd = np.zeros((len(src), 32), np.uint8)
    okr = (rows >= 0) & (rows < len(desc))
    qd[okr] = desc[rows[okr]]
    return q, qd, src, len(src), n_in_view, T


# ------------------------------------------------------------------------------------------------ scenes
def rot(rng, scale=0.3):
    w = rng.normal(0, scale, 3)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx).astype(f32)


def make_frame(R, t, Rl=None, tl=None, bounds=(0.0, W, 0.0, H)):
    F = np.zeros((), PROJECT_FRAME_DTYPE)
    F["Rcw"], F["tcw"] = np.asarray(R, f32).reshape(9), np.asarray(t, f32)
    F["Ow"] = mat_rows(-np.asarray(R, f32).T.reshape(9), np.asarray(t, f32)[None, :])[0]   # mOw = -Rcw.t()*tcw
    F["Rlw"] = np.asarray(Rl if Rl is not None else R, f32).reshape(9)
    F["tlw"] = np.asarray(tl if tl is not None else t, f32)
    F["bounds"] = np.asarray(bounds, f32)
    return F


def nudge_to(target, fn, x0, steps=64):
    """a float near x0 with fn(x) == target (fn monotone in x), else the closest tried"""
    x = f32(x0)
    for _ in range(steps):
        y = fn(x)
        if y == target:
            return x
        x = np.nextafter(x, f32(np.inf) if y < target else f32(-np.inf))
    return x


def make_scene(rng, mode, B, n, cap_mp, n_desc=None, special=True):
    """B frames x n map points, with the edge cases of the projection loops mixed in"""
    n_desc = n_desc or max(B * n // 2, 8)
    desc = rng.integers(0, 256, (n_desc, 32), dtype=np.uint8)
    mp = np.zeros((B, cap_mp), MAP_POINT_DTYPE)
    track = np.zeros((B, cap_mp), TRACK_DTYPE)
    frames = np.zeros(B, PROJECT_FRAME_DTYPE)
    nmp = np.full(B, n, np.int32)
    fx, fy, cx, cy = [float(c) for c in CAM]
    for b in range(B):
        R, t = rot(rng), rng.normal(0, 1.0, 3).astype(f32)
        # last-frame pose: the camera moved along its own z by -0.3 .. 0.3 (bForward / bBackward / neither)
        dz = [0.3, -0.3, 0.05, 0.0][b % 4]
        frames[b] = make_frame(R, t, R, (t + np.array([0, 0, dz])).astype(f32))
        uu, vv = rng.uniform(-60, W + 60, n), rng.uniform(-60, H + 60, n)
        z = rng.uniform(0.3, 25.0, n) * np.where(rng.random(n) < 0.1, -1, 1)
        Xc = np.stack([(uu - cx) / fx * z, (vv - cy) / fy * z, z], 1)
        Rd = R.astype(f64)
        X = ((Xc - t.astype(f64)) @ Rd).astype(f32)          # Rcw^T (Xc - tcw)
        m = mp[b, :n]
        m["pos"] = X
        PO = X.astype(f64) - frames[b]["Ow"].astype(f64)
        d = np.linalg.norm(PO, axis=1)
        dirn = PO / np.maximum(d, 1e-12)[:, None]
        # normals: a spread of viewing angles, many near cos = 0.5 and 0.998 (the isInFrustum limit and RadiusByViewingCos' switch)
        ang = np.where(rng.random(n) < 0.3, math.acos(0.5), np.where(rng.random(n) < 0.4, math.acos(0.998), rng.uniform(0, 2.0, n)))
        ang = ang + rng.normal(0, 2e-7, n)
        perp = np.cross(dirn, rng.normal(0, 1, (n, 3)))
        perp /= np.maximum(np.linalg.norm(perp, axis=1), 1e-12)[:, None]
        m["normal"] = (np.cos(ang)[:, None] * dirn + np.sin(ang)[:, None] * perp).astype(f32)
        lvl = rng.integers(0, NLEVELS, n)
        m["max_distance"] = (d * SF[lvl] * rng.uniform(0.7, 1.3, n)).astype(f32)
        m["min_distance"] = (m["max_distance"] / SF[NLEVELS - 1] * rng.uniform(0.8, 1.3, n)).astype(f32)
        m["angle"] = rng.uniform(0, 360, n).astype(f32)
        m["octave"] = rng.integers(0, NLEVELS, n)
        m["desc_row"] = rng.integers(0, n_desc, n)
        fl = np.full(n, MP_VALID, np.uint32)
        fl[rng.random(n) < 0.05] = 0
        fl[rng.random(n) < 0.08] |= MP_BAD
        fl[rng.random(n) < 0.6] |= MP_HAS_OBS
        if mode == PROJ_LOCAL_MAP:
            fl[rng.random(n) < 0.15] |= MP_SEEN
        m["flags"] = fl
        # stale track state from an earlier frame
        tr = track[b, :n]
        tr["in_view"] = rng.random(n) < 0.5
        tr["proj_x"], tr["proj_y"] = rng.uniform(0, W, n), rng.uniform(0, H, n)
        tr["proj_xr"], tr["depth"] = rng.uniform(-10, W, n), rng.uniform(0.1, 30, n)
        tr["view_cos"] = np.where(rng.random(n) < 0.5, f32(0.9985), f32(0.7))
        tr["level"] = rng.integers(0, NLEVELS, n)
        if special and n >= 40:
            _edge_cases(rng, mp[b], frames[b], n, m)
    if special and B >= 3 and mode == PROJ_LOCAL_MAP:
        # nToMatch == 0: nothing is visible, but stale SEEN entries are in view (the reference never calls the search)
        m = mp[2, :n]
        m["flags"] |= MP_SEEN
        track[2, :n]["in_view"] = 1
    if special and B >= 4:
        _zero_depth_frame(mp[3], frames, 3, n)
    if n_desc > 2 and special:
        mp[0, 1]["desc_row"] = -1      # out of range: gathers zeros
        mp[0, 2]["desc_row"] = n_desc
    return mp, nmp, desc, frames, track


def _edge_cases(rng, mpb, F, n, m):
    """points exactly on / one ulp outside the image bounds, distances exactly at the invariance limits"""
    X = np.ascontiguousarray(m["pos"])
    Pc, u, v, inside = project(X, F)
    front = np.nonzero((Pc[:, 2] > 0) & inside)[0]
    if len(front) < 12:
        return
    a, bb, c, d = front[np.argmin(u[front])], front[np.argmax(u[front])], front[np.argmin(v[front])], front[np.argmax(v[front])]
    front = np.setdiff1d(front, [a, bb, c, d])
    F["bounds"][0] = u[a]                                  # on the lower x bound: kept
    F["bounds"][1] = np.nextafter(u[bb], f32(-np.inf))     # one ulp outside the upper x bound
    F["bounds"][2] = np.nextafter(v[c], f32(np.inf))       # one ulp outside the lower y bound
    F["bounds"][3] = v[d]                                  # on the upper y bound: kept
    m["flags"][[a, bb, c, d]] = MP_VALID | MP_HAS_OBS
    PO = X - F["Ow"][None, :]
    dist = np.sqrt(dot3(PO, PO)).astype(f32)
    for k, i in enumerate(front[:6]):
        if k % 2 == 0:   # dist == 1.2f * mfMaxDistance (kept) / one ulp beyond
            mx = nudge_to(dist[i], lambda x: f32(1.2) * x, dist[i] / f32(1.2))
            m["max_distance"][i] = mx if k < 4 else np.nextafter(mx, f32(-np.inf))
            m["min_distance"][i] = f32(0)
        else:            # dist == 0.8f * mfMinDistance (kept) / one ulp inside
            mn = nudge_to(dist[i], lambda x: f32(0.8) * x, dist[i] / f32(0.8))
            m["min_distance"][i] = mn if k < 4 else np.nextafter(mn, f32(np.inf))
            m["max_distance"][i] = dist[i] * f32(2)
        m["flags"][i] = MP_VALID


def _zero_depth_frame(mpb, frames, b, n):
    """Rcw = diag(1, 1, 1e-30), tcw = (0, 0, -0): z = -0 (tiny negative products round to -0), +0, tiny positive, negative"""
    R = np.diag([1.0, 1.0, 1e-30]).astype(f32)
    F = make_frame(R, np.array([0.0, 0.0, -0.0], f32))
    F["tlw"] = np.array([0.0, 0.0, -0.0], f32)
    F["Rlw"] = R.reshape(9)
    frames[b] = F
    zs = [-1e-20, 1e-20, 1e20, -1e20, 5e29, 0.0]
    for k in range(min(24, n)):
        m = mpb[k]
        m["pos"] = np.array([[0.0, 1.0, -3.0, 0.5][k % 4], [0.0, -2.0, 0.0, 0.25][(k // 4) % 4] if k % 2 else 0.0, zs[k % len(zs)]], f32)
        m["min_distance"], m["max_distance"] = f32(0), f32(1e30)
        m["flags"] = MP_VALID | MP_HAS_OBS


# ------------------------------------------------------------------------------------------------ running the library
def params(m, mode, th, mono=True, far=False, th_far=0.0, view_cos_limit=0.5):
    return m.ProjectParams(mode, CAM, SF, LSF, th, mbf=MBF, mb=MB, bMono=mono, viewingCosLimit=view_cos_limit, bFarPoints=far,
                           thFarPoints=th_far)


def run(lib, backend, mp, nmp, desc, frames, track, prm, cap_q):
    m = orbhip.ORBmatcher(0.8, True, lib=lib)
    d_track = to_dev(track, backend) if prm.mode == PROJ_LOCAL_MAP else None
    if backend == "emu" and d_track is not None:
        d_track = track.copy()
    out = m.ProjectMapPoints(to_dev(mp, backend), to_dev_plain(nmp, backend), to_dev_plain(desc, backend), to_dev(frames, backend), prm, cap_q,
                             track=d_track)
    if backend == "hip":
        import torch
        torch.cuda.synchronize()
    return m, out


def check(lib, backend, mp, nmp, desc, frames, track, mode, th, cap_q, **kw):
    m = orbhip.ORBmatcher(0.8, True, lib=lib)
    prm = params(m, mode, th, **{k: v for k, v in kw.items() if k in ("mono", "far", "th_far", "view_cos_limit")})
    _, out = run(lib, backend, mp, nmp, desc, frames, track, prm, cap_q)
    Q = to_host(out["queries"]).reshape(len(nmp), cap_q, -1).view(QUERY_DTYPE)[..., 0]
    QD, NQ, SRC = to_host(out["qdesc"]), to_host(out["nq"]), to_host(out["q_src"])
    REQ, NIN = to_host(out["n_required"]), to_host(out["n_in_view"])
    T = to_host(out["track"]).reshape(track.shape + (-1,)).view(TRACK_DTYPE)[..., 0] if mode == PROJ_LOCAL_MAP else None
    stats = dict(queries=0, overflow=0, in_view=0)
    for b in range(len(nmp)):
        q, qd, src, req, nin, tr = ref_frame(mp[b], nmp[b], desc, frames[b], track[b] if mode == PROJ_LOCAL_MAP else None, mode, th,
                                             mono=kw.get("mono", True), far=kw.get("far", False), th_far=f32(kw.get("th_far", 0.0)),
                                             view_cos_limit=f32(kw.get("view_cos_limit", 0.5)))
        nq = min(req, cap_q)
        assert (REQ[b], NIN[b], NQ[b]) == (req, nin, nq), (b, REQ[b], NIN[b], NQ[b], req, nin, nq)
        assert np.array_equal(bits(Q[b, :nq]), bits(q[:nq])), (b, Q[b, :nq][:5], q[:nq][:5])
        assert np.array_equal(QD[b, :nq], qd[:nq]) and np.array_equal(SRC[b, :nq], src[:nq]), b
        if T is not None:
            assert np.array_equal(bits(T[b]), bits(np.concatenate([tr, track[b, nmp[b]:]]))), b
        stats["queries"] += nq
        stats["overflow"] += req > cap_q
        stats["in_view"] += nin
    return stats, out


# ------------------------------------------------------------------------------------------------ CPU tier (emulated library)
def test_local_map_emu(emu_lib):
    rng = np.random.default_rng(11)
    mp, nmp, desc, frames, track = make_scene(rng, PROJ_LOCAL_MAP, 5, 530, 540)
    nmp[4] = 300
    st, _ = check(emu_lib, "emu", mp, nmp, desc, frames, track, PROJ_LOCAL_MAP, 3.0, 540)
    assert st["queries"] > 400 and st["in_view"] > 300
    st, _ = check(emu_lib, "emu", mp, nmp, desc, frames, track, PROJ_LOCAL_MAP, 1.0, 540, far=True, th_far=8.0)   # th == 1: no factor
    assert st["queries"] > 100


def test_local_map_edge_coverage():
    """the scene really exercises the limits the kernel is compared on (restatement only)"""
    rng = np.random.default_rng(11)
    mp, nmp, desc, frames, track = make_scene(rng, PROJ_LOCAL_MAP, 5, 530, 540)
    X = np.ascontiguousarray(mp[0, :530]["pos"])
    PO = X - frames[0]["Ow"][None, :]
    dist = np.sqrt(dot3(PO, PO)).astype(f32)
    vc = (dot3(PO, np.ascontiguousarray(mp[0, :530]["normal"])) / dist.astype(f64)).astype(f32)
    assert (vc == f32(0.5)).any() and (vc == np.nextafter(f32(0.5), f32(0))).any()
    assert ((vc.astype(f64) > 0.998) & (vc < f32(0.9981))).any() and ((vc.astype(f64) <= 0.998) & (vc > f32(0.9979))).any()
    Pc, u, v, inside = project(X, frames[0])
    assert (u == frames[0]["bounds"][0]).any() and (v == frames[0]["bounds"][3]).any()
    assert (f32(1.2) * mp[0, :530]["max_distance"] == dist).any() and (f32(0.8) * mp[0, :530]["min_distance"] == dist).any()
    z = mat_rows(frames[3]["Rcw"], np.ascontiguousarray(mp[3, :24]["pos"]))[:, 2] + frames[3]["tcw"][2]
    assert ((z == 0) & np.signbit(z)).any() and ((z == 0) & ~np.signbit(z)).any()


def test_last_frame_emu(emu_lib):
    rng = np.random.default_rng(12)
    mp, nmp, desc, frames, track = make_scene(rng, PROJ_LAST_FRAME, 5, 300, 320)
    for mono in (True, False):
        st, _ = check(emu_lib, "emu", mp, nmp, desc, frames, track, PROJ_LAST_FRAME, 15.0, 320, mono=mono)
        assert st["queries"] > 500
    # bForward / bBackward / neither all occur among the frames
    dirs = set()
    for b in range(4):
        tz = mat_rows(frames[b]["Rlw"], frames[b]["Ow"][None, :])[0, 2] + frames[b]["tlw"][2]
        dirs.add(bool(tz > MB) - bool(-tz > MB))
    assert dirs == {-1, 0, 1}


def test_reloc_emu(emu_lib):
    rng = np.random.default_rng(13)
    mp, nmp, desc, frames, track = make_scene(rng, PROJ_RELOC, 5, 300, 300)
    st, _ = check(emu_lib, "emu", mp, nmp, desc, frames, track, PROJ_RELOC, 10.0, 300)
    assert st["queries"] > 300


def test_overflow_is_reported_emu(emu_lib):
    rng = np.random.default_rng(14)
    mp, nmp, desc, frames, track = make_scene(rng, PROJ_LAST_FRAME, 3, 300, 300)
    st, out = check(emu_lib, "emu", mp, nmp, desc, frames, track, PROJ_LAST_FRAME, 15.0, 17)
    assert st["overflow"] == 3
    m = orbhip.ORBmatcher(lib=emu_lib)
    with pytest.raises(OrbHipError) as e:
        m.check_overflow(out)
    assert e.value.code == ORB_E_CAPACITY
    _, out = check(emu_lib, "emu", mp, nmp, desc, frames, track, PROJ_LAST_FRAME, 15.0, 300)
    m.check_overflow(out)


def test_argument_errors_emu(emu_lib):
    rng = np.random.default_rng(15)
    mp, nmp, desc, frames, track = make_scene(rng, PROJ_LOCAL_MAP, 1, 50, 64, special=False)
    m = orbhip.ORBmatcher(lib=emu_lib)
    prm = params(m, PROJ_LOCAL_MAP, 1.0)

    def call(p=prm, cap_q=64, tr=track):
        return m._L.orbm_project_map_points(mp.ctypes.data, nmp.ctypes.data, 64, desc.ctypes.data, frames.ctypes.data, 1, ctypes.byref(p),
                                            None if tr is None else tr.ctypes.data, q.ctypes.data, qd.ctypes.data, cnt.ctypes.data,
                                            src.ctypes.data, cnt[1:].ctypes.data, cnt[2:].ctypes.data, cap_q, None)
    q, qd = np.zeros(64, QUERY_DTYPE), np.zeros((64, 32), np.uint8)
    src, cnt = np.zeros(64, np.int32), np.zeros(4, np.int32)
    assert call() == 0
    assert call(cap_q=0) == ORB_E_INVALID
    assert call(tr=None) == ORB_E_INVALID               # LOCAL_MAP needs the track states
    for field, bad in (("mode", 3), ("camera_type", 1), ("nleft", 100), ("nlevels", 17), ("nlevels", 0)):
        p = type(prm).from_buffer_copy(prm)
        setattr(p, field, bad)
        assert call(p) == ORB_E_INVALID, field
    assert m._L.orbm_predict_scale_thresholds(0.0, 8, q.ctypes.data) == ORB_E_INVALID
    assert m._L.orbm_predict_scale_thresholds(float(LSF), 17, q.ctypes.data) == ORB_E_INVALID


def sweep_records(lsf, nlevels, thresholds, span=2048):
    """one RELOC record per ratio bit pattern within +-span ulps of every level threshold: camera at the origin, point at (0, 0, 1), so that
    dist3D = 1 and ratio = mfMaxDistance exactly"""
    pats = np.concatenate([np.arange(-span, span + 1) + np.int64(np.float32(t).view(np.uint32)) for t in thresholds])
    ratios = pats.astype(np.uint32).view(np.float32)
    n = len(ratios)
    mp = np.zeros((1, n), MAP_POINT_DTYPE)
    mp["pos"] = np.array([0, 0, 1], f32)
    mp["max_distance"] = ratios
    mp["flags"] = MP_VALID
    frames = make_frame(np.eye(3), np.zeros(3))[None]
    return mp, np.array([n], np.int32), np.zeros((1, 32), np.uint8), frames, ratios


def _check_sweep(lib, backend, scale, nlevels):
    m = orbhip.ORBmatcher(lib=lib)
    lsf = f32(math.log(f32(scale)))
    thr = m.PredictScaleThresholds(lsf, nlevels)
    assert len(thr) == nlevels - 1 and np.all(np.diff(thr) > 0)
    mp, nmp, desc, frames, ratios = sweep_records(lsf, nlevels, thr)
    # the host logf is monotone over every sweep, and the step lies exactly on the threshold
    ref = predict_scale(ratios, lsf, nlevels)
    for k in range(nlevels - 1):
        seg = ref[k * 4097:(k + 1) * 4097]
        lg = np.array([logf(r) for r in ratios[k * 4097:(k + 1) * 4097]])
        assert np.all(np.diff(lg) >= 0) and np.all(np.diff(seg) >= 0)
        assert seg[2047] == k and seg[2048] == k + 1
    sf = np.array([f32(scale) ** i for i in range(nlevels)], np.float32)
    prm = m.ProjectParams(PROJ_RELOC, CAM, sf, lsf, 1.0)
    _, out = run(lib, backend, mp, nmp, desc, frames, None, prm, len(ratios))
    Q = to_host(out["queries"]).reshape(len(ratios), -1).view(QUERY_DTYPE)[:, 0]
    assert to_host(out["nq"])[0] == len(ratios)
    assert np.array_equal(Q["min_level"] + 1, ref)


@pytest.mark.parametrize("scale,nlevels", [(1.2, 8), (2.0, 4), (1.05, 16)])
def test_predict_scale_threshold_sweep_emu(emu_lib, scale, nlevels):
    _check_sweep(emu_lib, "emu", scale, nlevels)


# ---- chaining: projection -> orbm_search_by_projection on the device == the existing search fed host-built queries
def frame_for(rng, mp, nmp, frames, desc, cap_k, mode=PROJ_LAST_FRAME):
    """a current frame whose keypoints sit near the projections of most map points, descriptors a few bits off the map points'"""
    B = len(nmp)
    kps = np.zeros((B, cap_k), KP_DTYPE)
    kdesc = np.zeros((B, cap_k, 32), np.uint8)
    nk = np.zeros(B, np.int32)
    for b in range(B):
        X = np.ascontiguousarray(mp[b, :nmp[b]]["pos"])
        Pc, u, v, inside = project(X, frames[b])
        idx = np.nonzero(inside & (Pc[:, 2] > 0))[0]
        idx = idx[rng.random(len(idx)) < 0.8][:cap_k - 20]
        k = len(idx) + 20
        kps[b, :len(idx)]["x"] = u[idx] + rng.normal(0, 1.5, len(idx)).astype(f32)
        kps[b, :len(idx)]["y"] = v[idx] + rng.normal(0, 1.5, len(idx)).astype(f32)
        kps[b, len(idx):k]["x"], kps[b, len(idx):k]["y"] = rng.uniform(0, W, 20), rng.uniform(0, H, 20)
        if mode == PROJ_LAST_FRAME:
            octv = mp[b, idx]["octave"]
        else:   # the level PredictScale gives the point
            PO = X[idx] - frames[b]["Ow"][None, :]
            octv = predict_scale(mp[b, idx]["max_distance"] / np.sqrt(dot3(PO, PO)).astype(f32))
        kps[b, :k]["octave"] = np.concatenate([octv, rng.integers(0, NLEVELS, 20)])
        kps[b, :k]["angle"] = rng.uniform(0, 360, k)
        rows = np.clip(mp[b, idx]["desc_row"], 0, len(desc) - 1)
        d = desc[rows].copy()
        flip = rng.integers(0, 32, (len(idx), 3))
        for j in range(3):
            d[np.arange(len(idx)), flip[:, j]] ^= np.uint8(1 << j)
        kdesc[b, :len(idx)] = d
        kdesc[b, len(idx):k] = rng.integers(0, 256, (20, 32))
        nk[b] = k
    return kps.view(np.float32).reshape(B, cap_k, 7), kdesc, nk


def _chain(lib, backend, mode, th, seed, B, n, cap_q):
    rng = np.random.default_rng(seed)
    mp, nmp, desc, frames, track = make_scene(rng, mode, B, n, n, special=False)
    kps, kdesc, nk = frame_for(rng, mp, nmp, frames, desc, n + 40, mode)
    occ = (rng.random(kps.shape[:2]) < 0.05).astype(np.uint8)
    m = orbhip.ORBmatcher(0.8 if mode == PROJ_LOCAL_MAP else 0.9, True, lib=lib)
    prm = params(m, mode, th, mono=True)
    th_dist = 64 if mode == PROJ_RELOC else TH_HIGH
    dv = lambda a: to_dev_plain(a, backend)   # noqa: E731
    gs, gi = m.grid_build(dv(kps), dv(nk), GRID)
    d_track = track.copy() if backend == "emu" else to_dev(track, backend)
    res = m.SearchByProjectionFromMap(dv(kps), dv(kdesc), dv(nk), gs, gi, GRID, to_dev(mp, backend), dv(nmp), dv(desc), to_dev(frames, backend),
                                      prm, cap_q, track=d_track if mode == PROJ_LOCAL_MAP else None, th_dist=th_dist, occupied0=dv(occ))
    # the same search fed the restatement's queries
    qs = np.zeros((B, cap_q), QUERY_DTYPE)
    qd = np.zeros((B, cap_q, 32), np.uint8)
    nq = np.zeros(B, np.int32)
    srcs = []
    for b in range(B):
        q, d, src, req, _, _ = ref_frame(mp[b], nmp[b], desc, frames[b], track[b], mode, th)
        nq[b] = min(req, cap_q)
        qs[b, :nq[b]], qd[b, :nq[b]] = q[:nq[b]], d[:nq[b]]
        srcs.append(src)
    smode = MODE_LOCAL_MAP if mode == PROJ_LOCAL_MAP else MODE_BEST_ONLY
    qm, km, nm = m.SearchByProjection(dv(kps), dv(kdesc), dv(nk), gs, gi, dv(qs.view(np.uint8).reshape(B, cap_q, -1)), dv(qd), dv(nq), GRID, smode,
                                      th_dist, occupied0=dv(occ))
    qm, km, nm = to_host(qm), to_host(km), to_host(nm)
    assert np.array_equal(to_host(res["nmatches"]), nm) and nm.sum() > 20 * B, (to_host(res["nmatches"]), nm)
    assert np.array_equal(to_host(res["kp_match"]), km)
    for b in range(B):
        assert np.array_equal(to_host(res["q_match"])[b, :nq[b]], qm[b, :nq[b]])
        want = np.where(km[b] >= 0, srcs[b][np.maximum(km[b], 0)] if len(srcs[b]) else -1, km[b])
        assert np.array_equal(to_host(res["kp_match_mp"])[b], want)
    return res


@pytest.mark.parametrize("mode,th", [(PROJ_LOCAL_MAP, 3.0), (PROJ_LAST_FRAME, 15.0), (PROJ_RELOC, 10.0)])
def test_chained_search_emu(emu_lib, mode, th):
    _chain(emu_lib, "emu", mode, th, 21 + mode, 2, 300, 300)


# ------------------------------------------------------------------------------------------------ GPU tier (the product library)
@pytest.mark.gpu
def test_last_frame_512x1000_hip(hip_lib):
    rng = np.random.default_rng(31)
    mp, nmp, desc, frames, track = make_scene(rng, PROJ_LAST_FRAME, 512, 1000, 1000)
    for mono in (True, False):
        st, _ = check(hip_lib, "hip", mp, nmp, desc, frames, track, PROJ_LAST_FRAME, 15.0, 1000, mono=mono)
        assert st["queries"] > 512 * 300


@pytest.mark.gpu
@pytest.mark.parametrize("B", [64, 1])
def test_local_map_6000_hip(hip_lib, B):
    rng = np.random.default_rng(32 + B)
    mp, nmp, desc, frames, track = make_scene(rng, PROJ_LOCAL_MAP, B, 6000, 6000)
    st, _ = check(hip_lib, "hip", mp, nmp, desc, frames, track, PROJ_LOCAL_MAP, 3.0, 6000)
    assert st["queries"] > B * 1500
    st, _ = check(hip_lib, "hip", mp, nmp, desc, frames, track, PROJ_LOCAL_MAP, 1.0, 6000, far=True, th_far=8.0)


@pytest.mark.gpu
def test_reloc_and_overflow_hip(hip_lib):
    rng = np.random.default_rng(34)
    mp, nmp, desc, frames, track = make_scene(rng, PROJ_RELOC, 64, 1000, 1000)
    st, _ = check(hip_lib, "hip", mp, nmp, desc, frames, track, PROJ_RELOC, 10.0, 1000)
    assert st["queries"] > 64 * 200
    st, out = check(hip_lib, "hip", mp, nmp, desc, frames, track, PROJ_RELOC, 10.0, 64)
    assert st["overflow"] > 0
    with pytest.raises(OrbHipError):
        orbhip.ORBmatcher(lib=hip_lib).check_overflow(out)


@pytest.mark.gpu
@pytest.mark.parametrize("scale,nlevels", [(1.2, 8), (2.0, 4), (1.05, 16)])
def test_predict_scale_threshold_sweep_hip(hip_lib, scale, nlevels):
    _check_sweep(hip_lib, "hip", scale, nlevels)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,th", [(PROJ_LOCAL_MAP, 3.0), (PROJ_LAST_FRAME, 15.0), (PROJ_RELOC, 10.0)])
def test_chained_search_hip(hip_lib, mode, th):
    _chain(hip_lib, "hip", mode, th, 41 + mode, 16, 1000, 1000)


@pytest.mark.gpu
def test_graph_capture_replay_hip(hip_lib):
    """projection + search captured on one stream and replayed once == the eager call (the track state reset in between)"""
    import torch
    rng = np.random.default_rng(51)
    B, n = 32, 1500
    mp, nmp, desc, frames, track = make_scene(rng, PROJ_LOCAL_MAP, B, n, n, special=False)
    kps, kdesc, nk = frame_for(rng, mp, nmp, frames, desc, n + 40, PROJ_LOCAL_MAP)
    m = orbhip.ORBmatcher(0.8, True, lib=hip_lib)
    prm = params(m, PROJ_LOCAL_MAP, 3.0)
    dv = lambda a: to_dev_plain(a, "hip")   # noqa: E731
    d_kps, d_desc, d_nk = dv(kps), dv(kdesc), dv(nk)
    d_mp, d_nmp, d_mpd, d_fr = to_dev(mp, "hip"), dv(nmp), dv(desc), to_dev(frames, "hip")
    track0 = to_dev(track, "hip")
    d_track = track0.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gs, gi = m.grid_build(d_kps, d_nk, GRID)
        work = torch.empty(m._L.orbm_search_workspace_bytes(B, n), dtype=torch.uint8, device="cuda")
        res = m.SearchByProjectionFromMap(d_kps, d_desc, d_nk, gs, gi, GRID, d_mp, d_nmp, d_mpd, d_fr, prm, n, track=d_track, work=work)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in res.items() if hasattr(v, "clone")}
    assert int(eager["nmatches"].sum()) > 20 * B
    d_track.copy_(track0)
    for k in ("q_match", "kp_match", "kp_match_mp", "nmatches", "nq", "queries"):
        res[k].fill_(90)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.SearchByProjectionFromMap(d_kps, d_desc, d_nk, gs, gi, GRID, d_mp, d_nmp, d_mpd, d_fr, prm, n, track=d_track, work=work, out=res)
    d_track.copy_(track0)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        if k == "queries" or k == "qdesc" or k == "q_src" or k == "q_match":   # only the first nq entries are defined
            nq = eager["nq"].cpu().numpy()
            a, b_ = v.cpu().numpy(), res[k].cpu().numpy()
            for b in range(B):
                assert np.array_equal(a[b, :nq[b]], b_[b, :nq[b]]), (k, b)
        else:
            assert torch.equal(v, res[k]), k
