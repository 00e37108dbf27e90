"""New map points on the device (orbm_create_new_map_points, orbm_append_new_map_points) against a literal restatement of the loop they replace,
LocalMapping::CreateNewMapPoints (LocalMapping.cc:651-904), written below under rule R6 of DESIGN.md section 2: numpy float32 / float64 scalars
one operation at a time, math.atan2 / cos / tan (glibc) for the double transcendentals, the 4x4 null vector as rule R4 states it.

Compared bit for bit (NaN by class): d_status, d_new[:nnew], d_nnew, d_nrequired, d_point_of_1, d_point_of_2, both has_mp arrays, the pair
flags; for the append the map-point records, the observation CSR, the refresh records, the selection, the cursor and the counts.
backend "emu": the product kernels compiled against tests/emu; "hip": the real library on an MI355X."""
import math

import numpy as np
import pytest

import orbhip
from devarrays import BACKENDS, bits, lib, to_dev, to_dev_plain, to_host  # noqa: F401
from orbhip import KP_DTYPE
from orbhip._lib import ORB_E_CAPACITY, ORB_E_INVALID, OrbHipError, ptr
from orbhip.matcher import (KEYFRAME_CENTER_DTYPE, MAP_POINT_DTYPE, MP_HAS_OBS, MP_VALID, NEW_POINT_DTYPE, NEWPT_BAD_INDEX, NEWPT_BEHIND_1,
                            NEWPT_BEHIND_2, NEWPT_CAM_KB8, NEWPT_CAM_PINHOLE, NEWPT_CREATED_STEREO1, NEWPT_CREATED_STEREO2,
                            NEWPT_CREATED_TRIANGULATED, NEWPT_EMPTY_STEREO, NEWPT_FAR, NEWPT_LOW_PARALLAX, NEWPT_NO_MATCH, NEWPT_PAIR_BAD_CAMERA,
                            NEWPT_PAIR_BAD_INDEX, NEWPT_PAIR_DTYPE, NEWPT_PAIR_OVERFLOW, NEWPT_REPROJ_1, NEWPT_REPROJ_2, NEWPT_SCALE, NEWPT_W_ZERO,
                            NEWPT_ZERO_DIST, OBSERVATION_DTYPE, REFRESH_DESCRIPTOR, REFRESH_NORMAL_DEPTH, REFRESH_POINT_DTYPE, TRI_PAIR_DTYPE,
                            newpt_camera, newpt_pair)
from test_map_projection import CAM, MB, MBF, SF
from test_map_refresh import Scene
from test_map_refresh import expected as refresh_expected

F, D = np.float32, np.float64
SIGMA2 = (SF * SF).astype(F)                                  # mvLevelSigma2
KB8 = np.array([190.97847, 190.97331, 254.93171, 256.89744, 0.0034823894, 0.0007150348, -0.0020532361, 0.00020293673], F)   # a TUM-VI camera
CREATED = (NEWPT_CREATED_TRIANGULATED, NEWPT_CREATED_STEREO1, NEWPT_CREATED_STEREO2)
SENTINEL = 77


def nbits(rec):
    """devarrays.bits with the NaNs of sub-array float fields (pos[3], normal[3]) made the same too"""
    rec = np.array(rec, copy=True)
    for name in rec.dtype.names:
        if rec.dtype[name].base == np.float32:
            rec[name][np.isnan(rec[name])] = np.float32(np.nan)
    return bits(rec)


# ---------------------------------------------------------------------------------------------------- the restatement (rule R6)
def gemm3(a0, a1, a2, x, c=D(0)):
    """one element of a cv::gemm on floats with an addend: the double sum of the double products from 0 in k order, plus c, rounded once"""
    s = D(0)
    s = s + D(a0) * D(x[0])
    s = s + D(a1) * D(x[1])
    s = s + D(a2) * D(x[2])
    return F(s + D(c))


def ddot3(a, b):
    s = D(0)
    for k in range(3):
        s = s + D(a[k]) * D(b[k])
    return s


def _tan(x):
    return math.tan(x) if math.isfinite(x) else math.nan


def _cos(x):
    return math.cos(x) if math.isfinite(x) else math.nan


def _sin(x):
    return math.sin(x) if math.isfinite(x) else math.nan


def kb8_unproject(p, u, v):
    """KannalaBrandt8.cpp:101-124 under rule R4"""
    pwx, pwy = (u - p[2]) / p[0], (v - p[3]) / p[1]
    scale = F(1)
    theta_d = np.sqrt(pwx * pwx + pwy * pwy)
    half_pi = F(math.pi / 2)
    theta_d = max(-half_pi, theta_d)       # fmaxf: a NaN gives the other operand
    theta_d = min(theta_d, half_pi) if theta_d == theta_d else theta_d
    if D(theta_d) > 1e-8:
        theta = theta_d
        for _ in range(10):
            t2 = theta * theta
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t4 * t4
            k0, k1, k2, k3 = p[4] * t2, p[5] * t4, p[6] * t6, p[7] * t8
            fix = (theta * (F(1) + k0 + k1 + k2 + k3) - theta_d) / (F(1) + F(3) * k0 + F(5) * k1 + F(7) * k2 + F(9) * k3)
            theta = theta - fix
            if abs(fix) < F(1e-6):
                break
        scale = F(_tan(float(theta))) / theta_d
    return [pwx * scale, pwy * scale, F(1)]


def kb8_project(p, X):
    """KannalaBrandt8.cpp:28-42 under rule R4"""
    x2y2 = X[0] * X[0] + X[1] * X[1]
    theta = F(math.atan2(float(np.sqrt(x2y2)), float(X[2])))
    psi = F(math.atan2(float(X[1]), float(X[0])))
    t2 = theta * theta
    t3 = theta * t2
    t5 = t3 * t2
    t7 = t5 * t2
    t9 = t7 * t2
    r = theta + p[4] * t3 + p[5] * t5 + p[6] * t7 + p[7] * t9
    return F(D(p[0] * r) * D(_cos(float(psi))) + D(p[2])), F(D(p[1] * r) * D(_sin(float(psi))) + D(p[3]))


def unproject(cam, u, v):
    k = cam["k"]
    if cam["camera_type"] == NEWPT_CAM_KB8:
        return kb8_unproject(k, u, v)
    return [(u - k[2]) / k[0], (v - k[3]) / k[1], F(1)]           # Pinhole.cpp:63-69


def project(cam, X):
    k = cam["k"]
    if cam["camera_type"] == NEWPT_CAM_KB8:
        return kb8_project(k, X)
    return k[0] * X[0] / X[2] + k[2], k[1] * X[1] / X[2] + k[3]   # Pinhole.cpp:31-35


def null_vector4(A):
    """the last row of cv::SVD's vt for a 4x4 CV_32F matrix as rule R4 states it: cyclic Jacobi on A^T A in double, 8 sweeps, the eigenvector of
    the least diagonal entry (the first of equals)"""
    M = [[D(0)] * 4 for _ in range(4)]
    V = [[D(1) if i == j else D(0) for j in range(4)] for i in range(4)]
    for i in range(4):
        for j in range(4):
            s = D(0)
            for k in range(4):
                s = s + D(A[k * 4 + i]) * D(A[k * 4 + j])
            M[i][j] = s
    for _ in range(8):
        for p in range(3):
            for q in range(p + 1, 4):
                apq = M[p][q]
                if apq == 0:
                    continue
                th = (M[q][q] - M[p][p]) / (D(2) * apq)
                t = (D(1) if th >= 0 else D(-1)) / (abs(th) + np.sqrt(th * th + D(1)))
                c = D(1) / np.sqrt(t * t + D(1))
                sn = t * c
                for k in range(4):
                    a, b = M[k][p], M[k][q]
                    M[k][p], M[k][q] = c * a - sn * b, sn * a + c * b
                for k in range(4):
                    a, b = M[p][k], M[q][k]
                    M[p][k], M[q][k] = c * a - sn * b, sn * a + c * b
                for k in range(4):
                    a, b = V[k][p], V[k][q]
                    V[k][p], V[k][q] = c * a - sn * b, sn * a + c * b
    m = 0
    for i in range(1, 4):
        if M[i][i] < M[m][m]:
            m = i
    return [F(V[k][m]) for k in range(4)]


def stereo_cos(mb, depth):
    """cos(2*atan2(mb/2, depth)) through the float overloads (LocalMapping.cc:758, 760)"""
    th = F(math.atan2(float(mb / F(2)), float(depth)))
    return F(_cos(float(F(2) * th)))


def unproject_stereo(cam, raw, z):
    """KeyFrame::UnprojectStereo (KeyFrame.cc:861-877); None = the empty cv::Mat"""
    if not z > 0:
        return None
    k, R = cam["k"], cam["Rcw"]
    xc = [(raw["x"] - k[2]) * z * cam["invfx"], (raw["y"] - k[3]) * z * cam["invfy"], z]
    return [gemm3(R[i], R[3 + i], R[6 + i], xc, cam["Ow"][i]) for i in range(3)]


def reproj_rejects(cam, mbf, x3D, z, kp, stereo, ur, sigma2):
    R, t, k = cam["Rcw"], cam["tcw"], cam["k"]
    x, y = gemm3(R[0], R[1], R[2], x3D, t[0]), gemm3(R[3], R[4], R[5], x3D, t[1])
    invz = F(D(1) / D(z))
    if not stereo:
        u, v = project(cam, [x, y, z])
        ex, ey = u - kp["x"], v - kp["y"]
        return bool(D(ex * ex + ey * ey) > D(5.991) * D(sigma2))
    u = k[0] * x * invz + k[2]
    u_r = u - mbf * invz
    v = k[1] * y * invz + k[3]
    ex, ey, er = u - kp["x"], v - kp["y"], u_r - ur
    return bool(D(ex * ex + ey * ey + er * er) > D(7.8) * D(sigma2))


def dist_to(x3D, Ow):
    d = [x3D[i] - Ow[i] for i in range(3)]
    return F(np.sqrt(ddot3(d, d)))


def create_one(P, S1, S2, i1, idx2, mbf2_own=False, trace=None):
    """LocalMapping.cc:653-904 for one match -> (exit code, x3D); mbf2_own: the second key frame's stereo gate with its own mbf, which the
    reference does NOT do (:856) — only to show that the data of a test tells the two apart"""
    c1, c2 = P["cam1"], P["cam2"]
    kp1, kp2 = S1["kps"][i1], S2["kps"][idx2]
    if not (0 <= kp1["octave"] < 16 and 0 <= kp2["octave"] < 16):
        return NEWPT_BAD_INDEX, None
    ur1 = S1["u_right"][i1] if S1.get("u_right") is not None else F(-1)
    ur2 = S2["u_right"][idx2] if S2.get("u_right") is not None else F(-1)
    st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)
    xn1, xn2 = unproject(c1, kp1["x"], kp1["y"]), unproject(c2, kp2["x"], kp2["y"])
    R1, R2 = c1["Rcw"], c2["Rcw"]
    ray1 = [gemm3(R1[i], R1[3 + i], R1[6 + i], xn1) for i in range(3)]
    ray2 = [gemm3(R2[i], R2[3 + i], R2[6 + i], xn2) for i in range(3)]
    cos_rays = F(ddot3(ray1, ray2) / (np.sqrt(ddot3(ray1, ray1)) * np.sqrt(ddot3(ray2, ray2))))
    if trace is not None:
        trace["cos_rays"] = cos_rays
    cs1 = cs2 = cos_rays + F(1)
    if st1:
        cs1 = stereo_cos(c1["mb"], S1["depth"][i1])
    elif st2:
        cs2 = stereo_cos(c2["mb"], S2["depth"][idx2])
    cos_stereo = cs2 if cs2 < cs1 else cs1                               # std::min
    if cos_rays < cos_stereo and cos_rays > 0 and (st1 or st2 or D(cos_rays) < D(0.9998)):
        t1, t2 = c1["tcw"], c2["tcw"]
        A = [F(0)] * 16
        for c in range(4):
            T1 = [R1[c], R1[3 + c], R1[6 + c]] if c < 3 else [t1[0], t1[1], t1[2]]
            T2 = [R2[c], R2[3 + c], R2[6 + c]] if c < 3 else [t2[0], t2[1], t2[2]]
            A[c] = xn1[0] * T1[2] - T1[0]
            A[4 + c] = xn1[1] * T1[2] - T1[1]
            A[8 + c] = xn2[0] * T2[2] - T2[0]
            A[12 + c] = xn2[1] * T2[2] - T2[1]
        v = null_vector4(A)
        if v[3] == 0:
            return NEWPT_W_ZERO, None
        x3D = [v[i] / v[3] for i in range(3)]
        how = NEWPT_CREATED_TRIANGULATED
    elif st1 and cs1 < cs2:
        x3D = unproject_stereo(c1, (S1["kps_raw"] if S1.get("kps_raw") is not None else S1["kps"])[i1], S1["depth"][i1])
        how = NEWPT_CREATED_STEREO1
    elif st2 and cs2 < cs1:
        x3D = unproject_stereo(c2, (S2["kps_raw"] if S2.get("kps_raw") is not None else S2["kps"])[idx2], S2["depth"][idx2])
        how = NEWPT_CREATED_STEREO2
    else:
        return NEWPT_LOW_PARALLAX, None
    if x3D is None:
        return NEWPT_EMPTY_STEREO, None
    z1 = gemm3(R1[6], R1[7], R1[8], x3D, c1["tcw"][2])
    if z1 <= 0:
        return NEWPT_BEHIND_1, None
    z2 = gemm3(R2[6], R2[7], R2[8], x3D, c2["tcw"][2])
    if z2 <= 0:
        return NEWPT_BEHIND_2, None
    if reproj_rejects(c1, c1["mbf"], x3D, z1, kp1, st1, ur1, c1["level_sigma2"][kp1["octave"]]):
        return NEWPT_REPROJ_1, None
    if reproj_rejects(c2, c2["mbf"] if mbf2_own else c1["mbf"], x3D, z2, kp2, st2, ur2, c2["level_sigma2"][kp2["octave"]]):
        return NEWPT_REPROJ_2, None
    d1, d2 = dist_to(x3D, c1["Ow"]), dist_to(x3D, c2["Ow"])
    if d1 == 0 or d2 == 0:
        return NEWPT_ZERO_DIST, None
    if P["far_points"] and (d1 >= P["th_far_points"] or d2 >= P["th_far_points"]):
        return NEWPT_FAR, None
    ratio_dist = d2 / d1
    ratio_octave = c1["scale_factors"][kp1["octave"]] / c2["scale_factors"][kp2["octave"]]
    if ratio_dist * P["ratio_factor"] < ratio_octave or ratio_dist > ratio_octave * P["ratio_factor"]:
        return NEWPT_SCALE, None
    return how, x3D


def restate_pair(P, S1, S2, match12, cap_new, **kw):
    """one pair -> dict of everything the kernel writes for it; S1 / S2: dict(kps [cap], n, u_right, depth, kps_raw, has_mp)"""
    cap1, cap2 = len(S1["kps"]), len(S2["kps"])
    n1, n2 = min(max(int(S1["n"]), 0), cap1), min(max(int(S2["n"]), 0), cap2)
    out = dict(status=np.zeros(cap1, np.uint8), new=np.zeros(cap_new, NEW_POINT_DTYPE), point_of_1=np.full(cap1, -1, np.int32),
               point_of_2=np.full(cap2, -1, np.int32), has_mp1=None if S1.get("has_mp") is None else S1["has_mp"].copy(),
               has_mp2=None if S2.get("has_mp") is None else S2["has_mp"].copy())
    flags, req = 0, 0
    types = (int(P["cam1"]["camera_type"]), int(P["cam2"]["camera_type"]))
    if any(t not in (NEWPT_CAM_PINHOLE, NEWPT_CAM_KB8) for t in types):
        out.update(nnew=0, nrequired=0, pair_flags=NEWPT_PAIR_BAD_CAMERA)
        return out
    with np.errstate(all="ignore"):
        for i1 in range(cap1):
            idx2 = int(match12[i1])
            if idx2 == -1:
                continue
            if i1 >= n1 or idx2 < 0 or idx2 >= n2:
                code, x3D = NEWPT_BAD_INDEX, None
            else:
                code, x3D = create_one(P, S1, S2, i1, idx2, **kw)
            out["status"][i1] = code
            if code == NEWPT_BAD_INDEX:
                flags |= NEWPT_PAIR_BAD_INDEX
            if code in CREATED:
                j, req = req, req + 1
                if j < cap_new:
                    out["new"][j] = (x3D, i1, idx2, code)
                    out["point_of_1"][i1] = j
                    out["point_of_2"][idx2] = j                          # the later pKF2->AddMapPoint wins
                    if out["has_mp1"] is not None:
                        out["has_mp1"][i1] = 1
                    if out["has_mp2"] is not None:
                        out["has_mp2"][idx2] = 1
    if req > cap_new:
        flags |= NEWPT_PAIR_OVERFLOW
    out.update(nnew=min(req, cap_new), nrequired=req, pair_flags=flags)
    return out


# ---------------------------------------------------------------------------------------------------- scenes
def rot(rng, sigma):
    w = rng.normal(0, sigma, 3)
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) if a == 0 else np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / a ** 2 * K @ K


def camera(R, Ow, kb8=False, mb=MB, mbf=MBF):
    """orbm_newpt_camera of a key frame at Ow with rotation R (world -> camera), float32 members as the KeyFrame holds them"""
    R32 = R.astype(F)
    tcw = (-(R32.astype(D) @ np.asarray(Ow, D))).astype(F)
    return newpt_camera(R32.reshape(9), tcw, np.asarray(Ow, F), KB8 if kb8 else np.array(CAM, F), mb, mbf, SIGMA2, SF,
                        NEWPT_CAM_KB8 if kb8 else NEWPT_CAM_PINHOLE)


def observe(cam, X):
    """noise-free key points of the world points X [n,3] in float64 arithmetic, rounded to float32 -> (u, v, z)"""
    Pc = X @ cam["Rcw"].astype(D).reshape(3, 3).T + cam["tcw"].astype(D)
    k = cam["k"].astype(D)
    if cam["camera_type"] == NEWPT_CAM_KB8:
        th = np.arctan2(np.hypot(Pc[:, 0], Pc[:, 1]), Pc[:, 2])
        psi = np.arctan2(Pc[:, 1], Pc[:, 0])
        r = th + k[4] * th ** 3 + k[5] * th ** 5 + k[6] * th ** 7 + k[7] * th ** 9
        return (k[0] * r * np.cos(psi) + k[2]).astype(F), (k[1] * r * np.sin(psi) + k[3]).astype(F), Pc[:, 2]
    return (k[0] * Pc[:, 0] / Pc[:, 2] + k[2]).astype(F), (k[1] * Pc[:, 1] / Pc[:, 2] + k[3]).astype(F), Pc[:, 2]


def side(cam, X, cap, stereo, rng, order=None, stereo_fraction=0.6):
    """the arrays of one key frame observing X (feature order[i] = point i); stereo: mvuRight / mvDepth for a fraction of the features"""
    n = len(X)
    order = np.arange(n) if order is None else order
    kps = np.zeros(cap, KP_DTYPE)
    u, v, z = observe(cam, X)
    kps["x"][order], kps["y"][order] = u, v
    kps["octave"][:n] = 0
    S = dict(kps=kps, n=n, u_right=None, depth=None, kps_raw=None, has_mp=np.zeros(cap, np.uint8), z=np.zeros(cap))
    S["z"][order] = z
    if stereo:
        S["u_right"], S["depth"] = np.full(cap, -1, F), np.full(cap, -1, F)
        has = rng.random(n) < stereo_fraction
        idx = order[has]
        S["depth"][idx] = z[has].astype(F)
        S["u_right"][idx] = (u[has] - cam["mbf"] / z[has].astype(F)).astype(F)
    return S


def make_pair(seed, n, kind="mm", pad=5, baseline=(0.1, 1.0), depth=(2.0, 10.0), wrong=0.2, unmatched=0.1, cap_pad2=9, **pair_kw):
    """Two key frames `baseline` m apart, n planted points `depth` m in front of the first, every point seen noise-free by both; match12 =
    the correct pairing, except `wrong` of the features paired with another feature and `unmatched` of them with none.
    kind: two letters of m (monocular pinhole), s (stereo pinhole), k (KannalaBrandt8)."""
    rng = np.random.default_rng(seed)
    R1, O1 = rot(rng, 0.05), rng.normal(0, 0.5, 3)
    d = rng.normal(size=3)
    d[2] *= 0.3
    O2 = O1 + R1.T @ (d / np.linalg.norm(d) * rng.uniform(*baseline))
    R2 = rot(rng, 0.03) @ R1
    c1, c2 = camera(R1, O1, kind[0] == "k"), camera(R2, O2, kind[1] == "k")
    z = rng.uniform(*depth, n)
    Xc = np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1)
    X = Xc @ R1 + O1                                                     # camera 1 -> world
    order2 = rng.permutation(n)
    cap1, cap2 = max(n, 1) + pad, max(n, 1) + cap_pad2
    S1, S2 = side(c1, X, cap1, kind[0] == "s", rng), side(c2, X, cap2, kind[1] == "s", rng, order2)
    oct1 = rng.integers(0, 8, n)
    S1["kps"]["octave"][:n] = oct1
    S2["kps"]["octave"][order2] = oct1
    m12 = np.full(cap1, -1, np.int32)
    m12[:n] = order2
    r = rng.random(n)
    bad = r < wrong
    m12[:n][bad] = rng.integers(0, max(n, 1), bad.sum())
    m12[:n][(r >= wrong) & (r < wrong + unmatched)] = -1
    P = newpt_pair(c1, c2, F(1.2), **pair_kw)
    return dict(P=P, S1=S1, S2=S2, m12=m12, X=X, order2=order2, correct=np.concatenate([~bad & (r >= wrong + unmatched), np.zeros(cap1 - n, bool)]))


# ---------------------------------------------------------------------------------------------------- running the library
def stack(cases, key, sub, cap, fill, dtype):
    if all(c[key].get(sub) is None for c in cases):
        return None
    out = np.full((len(cases), cap), fill, dtype) if dtype != KP_DTYPE else np.zeros((len(cases), cap), KP_DTYPE)
    for b, c in enumerate(cases):
        a = c[key].get(sub)
        if a is not None:
            out[b, :len(a)] = a
    return out


def batch_arrays(cases, with_has_mp=True):
    """the [B, cap] arrays of a list of cases (caps = the largest of the batch); a side that no case gives u_right is monocular (NULL)"""
    cap1, cap2 = max(len(c["S1"]["kps"]) for c in cases), max(len(c["S2"]["kps"]) for c in cases)
    sides = []
    for key, cap in (("S1", cap1), ("S2", cap2)):
        s = dict(kps=stack(cases, key, "kps", cap, 0, KP_DTYPE), kps_raw=stack(cases, key, "kps_raw", cap, 0, KP_DTYPE),
                 u_right=stack(cases, key, "u_right", cap, -1, F), depth=stack(cases, key, "depth", cap, -1, F),
                 n=np.array([c[key]["n"] for c in cases], np.int32), has_mp=stack(cases, key, "has_mp", cap, 0, np.uint8) if with_has_mp else None)
        sides.append(s)
    m12 = np.full((len(cases), cap1), -1, np.int32)
    for b, c in enumerate(cases):
        m12[b, :len(c["m12"])] = c["m12"]
    return sides[0], sides[1], np.array([c["P"] for c in cases], NEWPT_PAIR_DTYPE), m12


def host_side(s, b):
    return {k: (v if v is None else (int(v[b]) if k == "n" else v[b])) for k, v in s.items()}


def upload_side(s, backend):
    return {k: (to_dev(v, backend) if k in ("kps", "kps_raw") else to_dev_plain(v, backend)) for k, v in s.items()}


def compare(got, exp, where=""):
    """one pair's outputs, bit for bit"""
    assert np.array_equal(got["status"], exp["status"]), (where, np.nonzero(got["status"] != exp["status"])[0][:10],
                                                          got["status"][got["status"] != exp["status"]][:10], exp["status"][got["status"] != exp["status"]][:10])
    assert (got["nnew"], got["nrequired"], got["pair_flags"]) == (exp["nnew"], exp["nrequired"], exp["pair_flags"]), where
    n = exp["nnew"]
    assert np.array_equal(nbits(got["new"][:n]), nbits(exp["new"][:n])), (where, got["new"][:n], exp["new"][:n])
    for k in ("point_of_1", "point_of_2", "has_mp1", "has_mp2"):
        assert (got[k] is None and exp[k] is None) or np.array_equal(got[k], exp[k]), (where, k)


def run_create(lib, backend, cases, cap_new, with_has_mp=True):
    """one launch for the batch -> per pair the dict compare() takes"""
    s1, s2, pairs, m12 = batch_arrays(cases, with_has_mp)
    m = orbhip.ORBmatcher(lib=lib)
    d1, d2 = upload_side(s1, backend), upload_side(s2, backend)
    out = m.CreateNewMapPoints(d1, d2, to_dev(pairs, backend), to_dev_plain(m12, backend), cap_new)
    if backend == "hip":
        import torch
        torch.cuda.synchronize()
    h = {k: to_host(v) for k, v in out.items() if k != "cap_new"}
    h1, h2 = (None if d1["has_mp"] is None else to_host(d1["has_mp"])), (None if d2["has_mp"] is None else to_host(d2["has_mp"]))
    got = []
    for b in range(len(cases)):
        got.append(dict(status=h["status"][b], new=h["new"][b].reshape(-1).view(NEW_POINT_DTYPE), nnew=int(h["nnew"][b]),
                        nrequired=int(h["nrequired"][b]), pair_flags=int(h["pair_flags"][b]), point_of_1=h["point_of_1"][b],
                        point_of_2=h["point_of_2"][b], has_mp1=None if h1 is None else h1[b], has_mp2=None if h2 is None else h2[b]))
    return got, (s1, s2, pairs, m12), m, out


_EXPECTED = {}


def restated(key, cases, cap_new, with_has_mp=True):
    """the restatement of a batch, computed once per key (both backends of a case share it)"""
    if key not in _EXPECTED:
        s1, s2, pairs, m12 = batch_arrays(cases, with_has_mp)
        _EXPECTED[key] = [restate_pair(pairs[b], host_side(s1, b), host_side(s2, b), m12[b], cap_new) for b in range(len(cases))]
    return _EXPECTED[key]


def check(lib, backend, cases, cap_new, key, with_has_mp=True):
    """launch, restate, compare -> the restated outputs"""
    got, _, _, _ = run_create(lib, backend, cases, cap_new, with_has_mp)
    exp = restated(key, cases, cap_new, with_has_mp)
    for b in range(len(cases)):
        compare(got[b], exp[b], "pair %d" % b)
    return exp


# ---------------------------------------------------------------------------------------------------- sizes and branches
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n1", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes(lib, backend, n1):
    """every chunk and wave boundary of the ordered compaction, cap_f never a multiple of 64; stereo flags on a part of both sides"""
    c = make_pair(200 + n1, n1, "ss")
    assert len(c["S1"]["kps"]) % 64 and len(c["S2"]["kps"]) % 64
    exp = check(lib, backend, [c], max(n1, 1), key=("sizes", n1))[0]
    if n1 >= 63:
        assert exp["nnew"] > 0.3 * n1 and exp["nnew"] == exp["nrequired"]
        assert list(exp["new"]["idx1"][:exp["nnew"]]) == sorted(exp["new"]["idx1"][:exp["nnew"]])


@pytest.mark.parametrize("backend", BACKENDS)
def test_ragged_batch(lib, backend):
    """five pairs of different sizes and kinds in one launch"""
    cases = [make_pair(300 + i, n, kind) for i, (n, kind) in enumerate([(257, "mm"), (0, "ss"), (64, "sm"), (130, "ms"), (1, "mm")])]
    exp = check(lib, backend, cases, 200, key="ragged")
    assert exp[0]["nnew"] > 80 and exp[1]["nnew"] == 0 and exp[2]["nnew"] > 15 and exp[3]["nnew"] > 30


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", ["mm", "sm", "ms", "ss", "kk", "mk"])
def test_branches(lib, backend, kind):
    """mono-mono, the three stereo combinations, KannalaBrandt8-KannalaBrandt8 and pinhole-KannalaBrandt8"""
    c = make_pair(400 + sum(map(ord, kind)), 150, kind, baseline=(0.5, 1.0))
    exp = check(lib, backend, [c], 150, key=("branch", kind))[0]
    created = np.isin(exp["status"], CREATED)
    assert created[c["correct"]].mean() > 0.8 and created[~c["correct"]].mean() < 0.3, kind


@pytest.mark.parametrize("backend", BACKENDS)
def test_stereo_unprojection_branches(lib, backend):
    """near points on a tiny baseline: the rays' parallax is below the stereo parallax, so the point comes from UnprojectStereo of the first key
    frame, or of the second when the first has no depth for the feature (bStereo2's cosine exists only when !bStereo1, :757-760); kps_raw
    (mvKeys) differs from kps (mvKeysUn) and is what UnprojectStereo reads"""
    c = make_pair(501, 120, "ss", baseline=(0.005, 0.01), depth=(0.6, 1.5), wrong=0.0)
    for S in (c["S1"], c["S2"]):
        S["kps_raw"] = S["kps"].copy()
        S["kps_raw"]["x"] += F(0.25)
    exp = check(lib, backend, [c], 120, key="stereo_unproject")[0]
    st = exp["status"]
    assert (st == NEWPT_CREATED_STEREO1).sum() > 20 and (st == NEWPT_CREATED_STEREO2).sum() > 5
    raw_blind = dict(c, S1=dict(c["S1"], kps_raw=None), S2=dict(c["S2"], kps_raw=None))
    s1, s2, pairs, m12 = batch_arrays([raw_blind])
    other = restate_pair(pairs[0], host_side(s1, 0), host_side(s2, 0), m12[0], 120)
    assert not np.array_equal(nbits(other["new"]), nbits(exp["new"]))     # the data tells mvKeys from mvKeysUn


def exit_zoo():
    """pairs built to reach the exits a clean scene does not: far points, octave mismatch (scale), a camera centre placed on a created point
    (zero distance), depth 0 with u_right >= 0 (empty stereo), indices out of range, wide wrong pairings (behind either camera)"""
    far = make_pair(601, 80, "mm", bFarPoints=True, thFarPoints=F(5.0))
    scale = make_pair(602, 80, "mm", wrong=0.0)
    scale["S2"]["kps"]["octave"][scale["order2"][::3]] = 7
    scale["S1"]["kps"]["octave"][:80:3] = 0
    zero = make_pair(603, 40, "mm", wrong=0.0, unmatched=0.0)
    s1, s2, pairs, m12 = batch_arrays([zero])
    first = restate_pair(pairs[0], host_side(s1, 0), host_side(s2, 0), m12[0], 40)
    assert first["nnew"] > 30
    zero["P"]["cam2"]["Ow"] = first["new"][7]["pos"]                      # dist2 == 0 for that match; the record's Ow is what the kernel reads
    empty = make_pair(604, 60, "ss", wrong=0.0)
    for S, k in ((empty["S1"], 4), (empty["S2"], 5)):
        S["depth"][:60:k] = 0
        S["u_right"][:60:k] = np.abs(S["u_right"][:60:k])
    index = make_pair(605, 50, "mm")
    index["m12"][3], index["m12"][9], index["m12"][20] = 50, -2, 2 ** 31 - 1
    index["m12"][52] = 4                                                 # i1 >= n1
    index["m12"][30], index["m12"][31] = 5, 6
    index["S1"]["kps"]["octave"][30], index["S2"]["kps"]["octave"][6] = 16, -1
    behind = make_pair(606, 200, "mm", wrong=1.0, unmatched=0.0, baseline=(0.8, 1.0), depth=(1.0, 3.0))
    # points between the two cameras along the optical axis: in front of the first key frame, behind the second, whose (mirrored) key point
    # still defines a line through the point
    rng = np.random.default_rng(607)
    c1, c2 = camera(np.eye(3), np.zeros(3)), camera(np.eye(3), np.array([0.05, 0.02, 1.0]))
    z = rng.uniform(0.3, 0.8, 40)
    X = np.stack([rng.uniform(-0.4, 0.4, 40) * z, rng.uniform(-0.3, 0.3, 40) * z, z], 1)
    S1, S2 = side(c1, X, 45, False, rng), side(c2, X, 49, False, rng)
    S1["kps"]["octave"][:40] = S2["kps"]["octave"][:40] = 2
    between = dict(P=newpt_pair(c1, c2, F(1.2)), S1=S1, S2=S2, m12=np.concatenate([np.arange(40), np.full(5, -1)]).astype(np.int32))
    return [far, scale, zero, empty, index, behind, between]


@pytest.mark.parametrize("backend", BACKENDS)
def test_exit_zoo(lib, backend):
    exp = check(lib, backend, exit_zoo(), 200, key="zoo")
    st = [e["status"] for e in exp]
    assert (st[0] == NEWPT_FAR).sum() > 10 and (st[1] == NEWPT_SCALE).sum() > 10 and (st[2] == NEWPT_ZERO_DIST).sum() == 1
    assert (st[3] == NEWPT_EMPTY_STEREO).sum() > 5
    assert list(st[4][[3, 9, 20, 52, 30, 31]]) == [NEWPT_BAD_INDEX] * 6 and exp[4]["pair_flags"] == NEWPT_PAIR_BAD_INDEX
    assert all(e["pair_flags"] == 0 for e in exp[:4])
    assert (st[6] == NEWPT_BEHIND_2).sum() > 10
    for code in (NEWPT_BEHIND_1, NEWPT_REPROJ_1, NEWPT_REPROJ_2, NEWPT_LOW_PARALLAX):
        assert any((s == code).any() for s in st), code


def w_zero_case():
    """x3D.at<float>(3) == 0 exactly: both key points on the principal point, equal rotations, a translation along x.  A^T A then has a zero row
    and column 2 that no rotation touches, so the least eigenvector is (0, 0, 1, 0): the point at infinity.  The parallel rays (cosine 1) pass
    :765 because the second feature is stereo with a NaN depth: cosParallaxStereo2 is NaN, std::min keeps cosParallaxRays + 1."""
    c = make_pair(607, 4, "ms", wrong=0.0, unmatched=0.0)
    I3 = np.eye(3)
    c["P"]["cam1"], c["P"]["cam2"] = camera(I3, np.zeros(3)), camera(I3, np.array([0.5, 0, 0]))
    c["S1"]["kps"]["x"][0], c["S1"]["kps"]["y"][0] = CAM[2], CAM[3]
    j = c["m12"][0]
    c["S2"]["kps"]["x"][j], c["S2"]["kps"]["y"][j] = CAM[2], CAM[3]
    c["S2"]["u_right"][j], c["S2"]["depth"][j] = F(300), F(np.nan)
    return c


@pytest.mark.parametrize("backend", BACKENDS)
def test_w_zero(lib, backend):
    exp = check(lib, backend, [w_zero_case()], 4, key="w_zero")[0]
    assert exp["status"][0] == NEWPT_W_ZERO


# ---------------------------------------------------------------------------------------------------- flips
def nextf(x, k=1):
    return (F(x).view(np.int32) + np.int32(k)).view(F) if x > 0 else (F(x).view(np.int32) - np.int32(k)).view(F)


def bisect_f32(pred, lo, hi):
    """lo, hi positive floats with pred(lo) != pred(hi) -> adjacent floats (a, b), a < b, with pred(a) == pred(lo) != pred(b)"""
    a, b = int(F(lo).view(np.int32)), int(F(hi).view(np.int32))
    pa = pred(np.int32(a).view(F))
    assert pa != pred(np.int32(b).view(F))
    while b - a > 1:
        mid = (a + b) // 2
        if pred(np.int32(mid).view(F)) == pa:
            a = mid
        else:
            b = mid
    return np.int32(a).view(F), np.int32(b).view(F)


def one_match(seed=700, kind="mm", baseline=0.1, depth=5.0, oct1=2, oct2=2):
    """a single planted point seen by two key frames with equal orientation `baseline` m apart along x: the pair the flip searches vary"""
    rng = np.random.default_rng(seed)
    c1, c2 = camera(np.eye(3), np.zeros(3)), camera(np.eye(3), np.array([baseline, 0.01, 0.0]))
    X = np.array([[0.3, -0.2, depth]])
    S1, S2 = side(c1, X, 3, kind[0] == "s", rng, stereo_fraction=1.0), side(c2, X, 3, kind[1] == "s", rng, stereo_fraction=1.0)
    S1["kps"]["octave"][0], S2["kps"]["octave"][0] = oct1, oct2
    return dict(P=newpt_pair(c1, c2, F(1.2)), S1=S1, S2=S2, m12=np.array([0, -1, -1], np.int32))


def vary(case, what, value):
    c = dict(P=case["P"].copy(), S1=dict(case["S1"], kps=case["S1"]["kps"].copy()), S2=dict(case["S2"], kps=case["S2"]["kps"].copy()),
             m12=case["m12"])
    if what == "ratio_factor":
        c["P"]["ratio_factor"] = value
    else:
        c[what[0]]["kps"][what[1]][0] = value
    return c


def code_of(case, trace=None):
    with np.errstate(all="ignore"):
        return create_one(case["P"], case["S1"], case["S2"], 0, 0, trace=trace)[0]


def flip_cases():
    """pairs of cases one float32 step apart on either side of a bound, found by searching the restatement"""
    out = []
    # cosParallaxRays == float(0.9998) (> the double literal: not triangulated) and one ulp below (triangulated): the second key point's x
    base = one_match(baseline=0.1, depth=5.0)
    target = F(0.9998)

    def cos_at(x):
        t = {}
        code_of(vary(base, ("S2", "x"), x), t)
        return t["cos_rays"]
    x0 = base["S2"]["kps"]["x"][0]
    for goal in (target, nextf(target, -1)):
        a, b = bisect_f32(lambda x: cos_at(x) <= goal, x0 - F(30), x0 + F(10))    # moving the point left opens the angle
        x = a if cos_at(a) == goal else b
        assert cos_at(x) == goal, (goal, cos_at(a), cos_at(b))
        out.append(("cos", vary(base, ("S2", "x"), x)))
    assert D(target) > D(0.9998) and D(nextf(target, -1)) < D(0.9998)
    assert code_of(out[0][1]) == NEWPT_LOW_PARALLAX and code_of(out[1][1]) != NEWPT_LOW_PARALLAX
    # the reprojection gates: the key point's y one step inside / outside the chi-square bound, mono (5.991) and stereo (7.8), both key frames
    for kind in ("mm", "ss"):
        for sname, code in (("S1", NEWPT_REPROJ_1), ("S2", NEWPT_REPROJ_2)):
            # the error splits between the two views: the gate of the key frame with the finer level trips first
            good = one_match(kind=kind, baseline=0.5, oct1=0 if sname == "S1" else 3, oct2=3 if sname == "S1" else 0)
            y0 = good[sname]["kps"]["y"][0]
            a, b = bisect_f32(lambda y: code_of(vary(good, (sname, "y"), y)) not in CREATED, y0, y0 + F(40))
            assert code_of(vary(good, (sname, "y"), a)) in CREATED and code_of(vary(good, (sname, "y"), b)) == code and nextf(a) == b
            out += [("reproj", vary(good, (sname, "y"), a)), ("reproj", vary(good, (sname, "y"), b))]
    # ratioDist*ratioFactor < ratioOctave and ratioDist > ratioOctave*ratioFactor: ratio_factor one step either side, octaves 2 / 0 and 0 / 2
    for o1, o2 in ((2, 0), (0, 2)):
        good = one_match(baseline=0.5, oct1=o1, oct2=o2)
        a, b = bisect_f32(lambda r: code_of(vary(good, "ratio_factor", r)) == NEWPT_SCALE, F(1.01), F(3.0))
        assert code_of(vary(good, "ratio_factor", a)) == NEWPT_SCALE and code_of(vary(good, "ratio_factor", b)) in CREATED
        out += [("scale", vary(good, "ratio_factor", a)), ("scale", vary(good, "ratio_factor", b))]
    return out


_FLIPS = []


@pytest.mark.parametrize("backend", BACKENDS)
def test_flips(lib, backend):
    """the bounds, one float32 step either side: the parallax literal 0.9998 (a double), the chi-square gates, the scale-consistency gate"""
    if not _FLIPS:
        _FLIPS.extend(flip_cases())
    exp = check(lib, backend, [c for _, c in _FLIPS], 2, key="flips")
    codes = [int(e["status"][0]) for e in exp]
    assert codes[0] == NEWPT_LOW_PARALLAX and codes[1] in CREATED
    assert len(codes) == 2 + 8 + 4 and all((codes[i] in CREATED) != (codes[i + 1] in CREATED) for i in range(2, len(codes), 2))


@pytest.mark.parametrize("backend", BACKENDS)
def test_depth_zero_and_mbf(lib, backend):
    """depth exactly 0 with u_right >= 0 (the empty cv::Mat of UnprojectStereo); the two key frames' mbf differ and the second key frame's
    u2_r still uses the FIRST one's (:856): u_right of the second key frame was made with its own mbf, so the reference rejects what a
    corrected formula would accept"""
    zero = one_match(kind="ss")
    zero["S1"]["depth"][0] = 0
    assert code_of(zero) == NEWPT_EMPTY_STEREO
    c = make_pair(702, 120, "ss", wrong=0.0, unmatched=0.0)
    c["P"]["cam2"]["mbf"] = F(10.0)
    S2 = c["S2"]
    has = S2["u_right"] >= 0
    S2["u_right"][has] = (S2["kps"]["x"][has] - F(10.0) / S2["depth"][has]).astype(F)
    exp = check(lib, backend, [zero, c], 120, key="mbf")
    assert exp[0]["status"][0] == NEWPT_EMPTY_STEREO
    s1, s2, pairs, m12 = batch_arrays([zero, c])
    own = restate_pair(pairs[1], host_side(s1, 1), host_side(s2, 1), m12[1], 120, mbf2_own=True)
    assert (exp[1]["status"] == NEWPT_REPROJ_2).sum() > 20 and (own["status"] == NEWPT_REPROJ_2).sum() == 0


# ---------------------------------------------------------------------------------------------------- other inputs
@pytest.mark.parametrize("backend", BACKENDS)
def test_two_idx1_on_one_idx2(lib, backend):
    """SearchForTriangulation never marks vbMatched2: two features of KF1 on one of KF2, both created; the later AddMapPoint wins"""
    c = make_pair(801, 100, "mm", wrong=0.0, unmatched=0.0)
    rng = np.random.default_rng(801)
    X2 = np.concatenate([c["X"], c["X"][:30] * (1 + 1e-3 * rng.normal(size=(30, 1)))])   # 30 more features of KF1 on nearly the same rays
    S1 = side(c["P"]["cam1"], X2, 135, False, rng)
    S1["kps"]["octave"][:100], S1["kps"]["octave"][100:130] = c["S1"]["kps"]["octave"][:100], c["S1"]["kps"]["octave"][:30]
    m12 = np.full(135, -1, np.int32)
    m12[:100], m12[100:130] = c["m12"][:100], c["m12"][:30]
    c.update(S1=S1, m12=m12)
    exp = check(lib, backend, [c], 130, key="twice")[0]
    both = [i for i in range(30) if exp["point_of_1"][i] >= 0 and exp["point_of_1"][100 + i] >= 0]
    assert len(both) >= 10
    for i in both:
        assert exp["point_of_2"][m12[i]] == exp["point_of_1"][100 + i] > exp["point_of_1"][i]


@pytest.mark.parametrize("backend", BACKENDS)
def test_bad_inputs_are_flagged_not_followed(lib, backend):
    """match12 far out of range (never read through), NaN poses (the reference's comparisons are all false on NaN: points with NaN positions
    pass the gates exactly as there), a camera type outside the two"""
    wild = make_pair(802, 70, "ss")
    wild["m12"][:70:7] = [2 ** 31 - 1, -2 ** 31, 70, 10 ** 6, -7, 79, 2 ** 30, 71, -2, 12345]
    nan = make_pair(803, 70, "sm")
    nan["P"]["cam1"]["Rcw"][4] = np.nan
    nan["P"]["cam2"]["tcw"][2] = np.nan
    cam = make_pair(804, 70, "mm")
    cam["P"]["cam2"]["camera_type"] = 2
    exp = check(lib, backend, [wild, nan, cam], 70, key="bad")
    assert (exp[0]["status"][:70:7] == NEWPT_BAD_INDEX).all() and exp[0]["pair_flags"] == NEWPT_PAIR_BAD_INDEX and exp[0]["nnew"] > 20
    assert exp[2]["pair_flags"] == NEWPT_PAIR_BAD_CAMERA and (exp[2]["status"] == NEWPT_NO_MATCH).all() and exp[2]["nnew"] == 0
    m = orbhip.ORBmatcher(lib=lib)
    with pytest.raises(OrbHipError) as e:
        m.check_new_points(dict(nrequired=np.array([3]), pair_flags=np.array([NEWPT_PAIR_BAD_INDEX]), cap_new=5))
    assert e.value.code == ORB_E_INVALID
    for kw in (dict(camera_type=2), dict(rig=True)):                     # the wrappers refuse what the kernel does not cover
        with pytest.raises(OrbHipError) as e:
            newpt_camera(np.eye(3), np.zeros(3), np.zeros(3), CAM, **kw)
        assert e.value.code == ORB_E_INVALID


@pytest.mark.parametrize("backend", BACKENDS)
def test_cap_new_one_below_and_null_has_mp(lib, backend):
    """cap_new one below the required count: the last point is reported, not stored (no has_mp, no point_of entry); has_mp pointers NULL"""
    c = make_pair(805, 90, "sm")
    s1, s2, pairs, m12 = batch_arrays([c])
    full = restate_pair(pairs[0], host_side(s1, 0), host_side(s2, 0), m12[0], 90)
    req = full["nrequired"]
    assert req > 40
    exp = check(lib, backend, [c], req - 1, key="cap")[0]
    assert (exp["nnew"], exp["nrequired"], exp["pair_flags"]) == (req - 1, req, NEWPT_PAIR_OVERFLOW)
    last = full["new"][req - 1]
    assert exp["point_of_1"][last["idx1"]] == -1 and exp["has_mp1"][last["idx1"]] == 0 and exp["status"][last["idx1"]] in CREATED
    m = orbhip.ORBmatcher(lib=lib)
    with pytest.raises(OrbHipError) as e:
        m.check_new_points(dict(nrequired=np.array([req]), pair_flags=np.array([NEWPT_PAIR_OVERFLOW]), cap_new=req - 1))
    assert e.value.code == ORB_E_CAPACITY
    null = check(lib, backend, [c], 90, key="null_has_mp", with_has_mp=False)[0]
    assert null["has_mp1"] is None and null["nnew"] == req


@pytest.mark.parametrize("backend", BACKENDS)
def test_argument_errors(lib, backend):
    c = make_pair(806, 20, "ss")
    s1, s2, pairs, m12 = batch_arrays([c])
    m = orbhip.ORBmatcher(lib=lib)
    L = m._L
    from orbhip.matcher import _newpt_side
    d1, d2 = upload_side(s1, backend), upload_side(s2, backend)
    out = m.CreateNewMapPoints(d1, d2, to_dev(pairs, backend), to_dev_plain(m12, backend), 20)
    import ctypes
    a, b = _newpt_side(d1), _newpt_side(d2)
    dp, dm = to_dev(pairs, backend), to_dev_plain(m12, backend)
    args = [ctypes.byref(a), ctypes.byref(b), ptr(dp), ptr(dm), 1, ptr(out["status"]), ptr(out["new"]), 20,
            ptr(out["nnew"]), ptr(out["nrequired"]), ptr(out["point_of_1"]), ptr(out["point_of_2"]), ptr(out["pair_flags"]), None]
    assert L.orbm_create_new_map_points(*args) == 0
    for k in (0, 1, 2, 3, 5, 6, 8, 9, 10, 11, 12):
        bad = list(args)
        bad[k] = None
        assert L.orbm_create_new_map_points(*bad) == ORB_E_INVALID, k
    for k, v in ((4, -1), (7, 0)):
        bad = list(args)
        bad[k] = v
        assert L.orbm_create_new_map_points(*bad) == ORB_E_INVALID, k
    args[4] = 0
    assert L.orbm_create_new_map_points(*args) == 0                      # batch == 0: a successful no-op
    for field in ("kps", "n"):
        s = _newpt_side(d1)
        setattr(s, field, None)
        assert L.orbm_create_new_map_points(ctypes.byref(s), *args[1:]) == ORB_E_INVALID
    s = _newpt_side(d1)
    s.depth = None                                                       # u_right without depth
    assert L.orbm_create_new_map_points(ctypes.byref(s), *args[1:]) == ORB_E_INVALID
    s = _newpt_side(d1)
    s.cap_f = 0
    assert L.orbm_create_new_map_points(ctypes.byref(s), *args[1:]) == ORB_E_INVALID
    if backend == "hip":
        import torch
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- sanity guard on the restatement (CPU)
def test_restatement_recovers_the_planted_points():
    """not the yardstick: the restatement itself against the planted geometry.  Noise-free key points (float32), every correct match whose true
    parallax is at least 1 degree is CREATED and its position is the planted one within GUARD_BOUND relative."""
    worst = 0.0
    for seed, kind in ((901, "mm"), (902, "ss"), (903, "kk"), (904, "mk")):
        c = make_pair(seed, 150, kind, baseline=(0.5, 1.0))
        s1, s2, pairs, m12 = batch_arrays([c])
        exp = restate_pair(pairs[0], host_side(s1, 0), host_side(s2, 0), m12[0], 150)
        O1, O2 = pairs[0]["cam1"]["Ow"].astype(D), pairs[0]["cam2"]["Ow"].astype(D)
        n_checked = 0
        for i1 in np.nonzero(c["correct"])[0]:
            X = c["X"][i1]
            r1, r2 = X - O1, X - O2
            if np.degrees(np.arccos(r1 @ r2 / np.linalg.norm(r1) / np.linalg.norm(r2))) < 1.0:
                continue
            n_checked += 1
            assert exp["status"][i1] in CREATED, (kind, i1, exp["status"][i1])
            got = exp["new"][exp["point_of_1"][i1]]["pos"].astype(D)
            worst = max(worst, np.linalg.norm(got - X) / np.linalg.norm(r1))
        assert n_checked > 80, (kind, n_checked)
    print("worst relative position error: %.3g" % worst)
    assert worst < GUARD_BOUND, worst


GUARD_BOUND = 3.8e-5   # 10 x the worst error measured on the CPU at these scenes: 3.78e-06


# ---------------------------------------------------------------------------------------------------- the neighbour chain
def chain_scene():
    """one current key frame and three neighbours from the extractor scene of the matcher tests (frame B = frame A shifted by (6, -4) px): equal
    orientations, the neighbour displaced parallel to the image plane so that the shift is the parallax of points 5 / 4.6 / 5.4 m away"""
    from test_matcher_parity import feature_vector, scene
    S = scene()
    rng = np.random.default_rng(1001)
    cam = np.array([200.0, 200.0, S["W"] / 2, S["H"] / 2], F)
    sig2 = (S["scale"] * S["scale"]).astype(F)

    def tri_side(k, dsc, stereo):
        ids, st, fe = feature_vector(dsc, 60)
        ur = np.full(len(k), -1, F)
        if stereo:
            sel = rng.random(len(k)) < 0.3
            ur[sel] = (k["x"][sel] - F(8.0)).astype(F)
        return dict(kps=k, desc=dsc, u_right=ur, depth=np.where(ur >= 0, F(5.0), F(-1)).astype(F), has_mp=(rng.random(len(k)) < 0.3).astype(np.uint8),
                    node_id=ids, node_start=st, feat_idx=fe, n_nodes=len(ids), n=len(k))
    kf1 = tri_side(S["ka"], S["da"], True)
    tx, ty = S["shift"]
    F12 = np.array([[0, 0, ty], [0, 0, -tx], [-ty, tx, 0]], F) * F(0.01)
    ep = np.array([-1e4, -1e4], F)
    neigh = []
    for z in (5.0, 4.6, 5.4):
        O2 = np.array([-tx * z / 200.0, -ty * z / 200.0, 0.0])
        c1 = newpt_camera(np.eye(3), np.zeros(3), np.zeros(3), cam, F(0.1), F(40.0), sig2, S["scale"])
        c2 = newpt_camera(np.eye(3), (-O2).astype(F), O2.astype(F), cam, F(0.1), F(40.0), sig2, S["scale"])
        tri = np.zeros((), TRI_PAIR_DTYPE)
        tri["F12"], tri["ep"] = F12.reshape(9), ep
        tri["level_sigma2_2"][:8], tri["scale_factors_2"][:8] = sig2, S["scale"]
        neigh.append(dict(kf2=tri_side(S["kb"], S["db"], False), pair=newpt_pair(c1, c2, F(1.2), kf1=0, kf2=len(neigh) + 1), tri=tri, F12=F12, ep=ep))
    return kf1, neigh, sig2, S["scale"]


def restate_chain(kf1, neigh, sig2, scale, cap_new, stale=False):
    """the reference's neighbour loop: SearchForTriangulation (the existing oracle), then the restated creation, the current key frame's
    map-point flags carried from one neighbour to the next (stale: NOT carried, to show what a missing update would do)"""
    import oracle_lib as O
    has1 = kf1["has_mp"].copy()
    out = []
    for nb in neigh:
        m12, _ = O.search_for_triangulation(dict(kf1, has_mp=has1), nb["kf2"], nb["F12"], nb["ep"], sig2, scale, False, False, False)
        S1 = dict(kps=kf1["kps"], n=kf1["n"], u_right=kf1["u_right"], depth=kf1["depth"], has_mp=has1)
        S2 = dict(kps=nb["kf2"]["kps"], n=nb["kf2"]["n"], u_right=nb["kf2"]["u_right"], depth=nb["kf2"]["depth"], has_mp=nb["kf2"]["has_mp"])
        e = restate_pair(nb["pair"], S1, S2, m12, cap_new)
        e["m12"] = m12.copy()
        out.append(e)
        if not stale:
            has1 = e["has_mp1"]
    return out


@pytest.mark.parametrize("backend", BACKENDS)
def test_neighbour_chain(lib, backend):
    """search -> create -> search -> create -> search -> create through the product wrappers on one stream, no host copy in between"""
    kf1, neigh, sig2, scale = chain_scene()
    cap_new = 400
    exp = restate_chain(kf1, neigh, sig2, scale, cap_new)
    stale = restate_chain(kf1, neigh, sig2, scale, cap_new, stale=True)
    # a feature neighbour 1 triangulates and neighbour 2 would match again if has_mp1 were stale
    again = [i for i in range(kf1["n"]) if exp[0]["point_of_1"][i] >= 0 and stale[1]["m12"][i] >= 0 and exp[1]["m12"][i] == -1]
    assert len(again) >= 3 and all(e["nnew"] > 5 for e in exp)
    m = orbhip.ORBmatcher(0.6, False, lib=lib)

    def dev(s, cap):
        o = {}
        for k, v in s.items():
            if k in ("n_nodes", "n"):
                o[k] = to_dev_plain(np.array([v], np.int32), backend)
            elif k == "kps":
                a = np.zeros((1, cap), KP_DTYPE)
                a[0, :len(v)] = v
                o[k] = to_dev_plain(np.ascontiguousarray(a).view(F).reshape(1, cap, 7), backend)
            else:
                c = {"node_id": 70, "node_start": 71}.get(k, cap)
                a = np.zeros((1, c) + v.shape[1:], v.dtype)
                a[0, :len(v)] = v
                o[k] = to_dev_plain(a, backend)
        return o
    cap1, cap2 = kf1["n"] + 5, neigh[0]["kf2"]["n"] + 9
    d1 = dev(kf1, cap1)
    outs, d2s = [], []
    for nb in neigh:                                                     # nothing below reads the device
        d2 = dev(nb["kf2"], cap2)
        m12, _ = m.SearchForTriangulation(d1, d2, to_dev(np.array([nb["tri"]]), backend))
        outs.append((m12, m.CreateNewMapPoints(d1, d2, to_dev(np.array([nb["pair"]]), backend), m12, cap_new)))
        d2s.append(d2)
    if backend == "hip":
        import torch
        torch.cuda.synchronize()
    h1 = to_host(d1["has_mp"])[0]
    for k, ((m12, o), e) in enumerate(zip(outs, exp)):
        assert np.array_equal(to_host(m12)[0, :kf1["n"]], e["m12"]), k
        got = dict(status=to_host(o["status"])[0][:kf1["n"]], new=to_host(o["new"])[0].reshape(-1).view(NEW_POINT_DTYPE), nnew=int(to_host(o["nnew"])[0]),
                   nrequired=int(to_host(o["nrequired"])[0]), pair_flags=int(to_host(o["pair_flags"])[0]),
                   point_of_1=to_host(o["point_of_1"])[0][:kf1["n"]], point_of_2=to_host(o["point_of_2"])[0][:len(e["point_of_2"])],
                   has_mp1=e["has_mp1"], has_mp2=to_host(d2s[k]["has_mp"])[0][:len(e["has_mp2"])])
        compare(got, e, "neighbour %d" % k)
    assert np.array_equal(h1[:kf1["n"]], exp[-1]["has_mp1"])


# ---------------------------------------------------------------------------------------------------- append
def append_world(cases, created, cursor, cap_mp, n_desc_rows, cap_obs, cap_sel, obs_kf2_first=(), seed=1100):
    """the device map before the append (sentinel fill behind the cursor) and what it has to be after -> (before, after) dicts of host arrays"""
    rng = np.random.default_rng(seed)
    mp = np.frombuffer(rng.integers(0, 256, cap_mp * MAP_POINT_DTYPE.itemsize, dtype=np.uint8).tobytes(), MAP_POINT_DTYPE).copy()
    mp["pos"], mp["normal"] = rng.normal(size=(cap_mp, 3)), rng.normal(size=(cap_mp, 3))
    mp["min_distance"], mp["max_distance"], mp["angle"] = 1, 2, 3
    obs = np.full(cap_obs, SENTINEL, np.int32).repeat(3).view(OBSERVATION_DTYPE).copy()
    ref = np.full(cap_mp, SENTINEL, np.int32).repeat(2).view(REFRESH_POINT_DTYPE).copy()
    obs_start = np.full(cap_mp + 1, SENTINEL, np.int32)
    obs_start[:cursor + 1] = np.arange(cursor + 1) * 3
    before = dict(mp=mp, obs=obs, ref=ref, obs_start=obs_start, n_mp=np.array([cursor], np.int32), sel=np.full(cap_sel, SENTINEL, np.int32))
    after = {k: v.copy() for k, v in before.items()}
    total = sum(e["nnew"] for e in created)
    ob = int(obs_start[cursor]) if 0 <= cursor <= cap_mp else 0
    fit = max(0, min(total, cap_mp - cursor, n_desc_rows - cursor, (cap_obs - ob) // 2, cap_sel)) if 0 <= cursor <= cap_mp and 0 <= ob <= cap_obs else 0
    r = 0
    for b, (c, e) in enumerate(zip(cases, created)):
        P = c["P"]
        for j in range(e["nnew"]):
            if r >= fit:
                break
            p, np_ = cursor + r, e["new"][j]
            after["mp"][p] = (np_["pos"], 0, 0, 0, 0, 0, p, MP_VALID | MP_HAS_OBS)
            o1, o2 = (P["kf1"], P["desc_row0_1"] + np_["idx1"], 0), (P["kf2"], P["desc_row0_2"] + np_["idx2"], 0)
            after["obs"][ob + 2 * r], after["obs"][ob + 2 * r + 1] = (o2, o1) if P["obs_kf2_first"] else (o1, o2)
            after["obs_start"][p + 1] = ob + 2 * r + 2
            after["ref"][p] = (P["kf1"], c["S1"]["kps"]["octave"][np_["idx1"]])
            after["sel"][r] = p
            r += 1
    after["sel"][fit:] = -1
    after["n_mp"][0] = cursor + fit
    after["appended"] = np.array([fit, total - fit], np.int32)
    return before, after


def append_cases():
    cases = [make_pair(1101 + i, n, kind, kf1=0, kf2=i + 1, obs_kf2_first=i % 2 == 1, desc_row0_1=0, desc_row0_2=300 * (i + 1))
             for i, (n, kind) in enumerate([(100, "mm"), (0, "mm"), (40, "ss"), (130, "sm"), (3, "mm")])]
    s1, s2, pairs, m12 = batch_arrays(cases)
    return cases, [restate_pair(pairs[b], host_side(s1, b), host_side(s2, b), m12[b], 120) for b in range(len(cases))]


def run_append(lib, backend, cases, before, n_desc_rows, created_dev=None):
    s1, s2, pairs, m12 = batch_arrays(cases)
    m = orbhip.ORBmatcher(lib=lib)
    d1, d2, dp = upload_side(s1, backend), upload_side(s2, backend), to_dev(pairs, backend)
    created = created_dev or m.CreateNewMapPoints(d1, d2, dp, to_dev_plain(m12, backend), 120)
    D_ = dict(mp=to_dev(before["mp"].copy(), backend), obs=to_dev(before["obs"].copy(), backend), ref=to_dev(before["ref"].copy(), backend),
              obs_start=to_dev_plain(before["obs_start"].copy(), backend), n_mp=to_dev_plain(before["n_mp"].copy(), backend))
    out = dict(sel=to_dev_plain(before["sel"].copy(), backend), appended=to_dev_plain(np.full(2, SENTINEL, np.int32), backend))
    m.AppendNewMapPoints(created, dp, d1["kps"], D_["n_mp"], D_["mp"], n_desc_rows, D_["obs_start"], D_["obs"], D_["ref"], len(before["sel"]), out=out)
    if backend == "hip":
        import torch
        torch.cuda.synchronize()
    return m, D_, out


def compare_append(D_, out, after):
    assert list(to_host(out["appended"])) == list(after["appended"]) and int(to_host(D_["n_mp"])[0]) == int(after["n_mp"][0])
    assert np.array_equal(to_host(out["sel"]), after["sel"])
    assert np.array_equal(to_host(D_["obs_start"]), after["obs_start"])
    assert np.array_equal(nbits(to_host(D_["mp"]).reshape(-1).view(MAP_POINT_DTYPE)), nbits(after["mp"]))
    assert np.array_equal(to_host(D_["obs"]).reshape(-1).view(np.int32), after["obs"].view(np.int32))
    assert np.array_equal(to_host(D_["ref"]).reshape(-1).view(np.int32), after["ref"].view(np.int32))


APPEND_ROOMY = dict(cursor=37, cap_mp=400, n_desc_rows=400, cap_obs=1000, cap_sel=300)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("short", [None, "cap_mp", "n_desc_rows", "cap_obs", "cap_sel", "cursor"])
def test_append(lib, backend, short):
    """cursor, record order across a ragged batch, the CSR tail, the selection's padding, both observation orders, every capacity shortfall;
    records that are not appended keep their bytes (sentinel fill)"""
    cases, created = append_cases()
    total = sum(e["nnew"] for e in created)
    assert total > 150 and created[1]["nnew"] == 0
    caps = dict(APPEND_ROOMY)
    if short == "cursor":
        caps["cursor"] = caps["cap_mp"] + 1                              # an impossible cursor: nothing is written, everything is counted short
    elif short == "cap_obs":
        caps[short] = 37 * 3 + 2 * 60 + 1
    elif short is not None:
        caps[short] = 60 if short == "cap_sel" else 37 + 60
    if short == "cursor":
        before, after = append_world(cases, created, 37, **{k: v for k, v in caps.items() if k != "cursor"})
        before["n_mp"][0] = after["n_mp"][0] = caps["cursor"]
        for k in ("mp", "obs", "ref", "obs_start"):
            after[k] = before[k].copy()
        after["sel"][:] = -1
        after["appended"] = np.array([0, total], np.int32)
    else:
        before, after = append_world(cases, created, **caps)
        assert after["appended"][0] == (total if short is None else 60)
    m, D_, out = run_append(lib, backend, cases, before, caps["n_desc_rows"])
    compare_append(D_, out, after)
    if short is not None:
        with pytest.raises(OrbHipError) as e:
            m.check_appended(out)
        assert e.value.code == ORB_E_CAPACITY
    else:
        m.check_appended(out)
        o = after["obs"][37 * 3:37 * 3 + 2 * total].reshape(-1, 2)
        first = np.repeat([c["P"]["obs_kf2_first"] for c in cases], [e["nnew"] for e in created])
        assert np.array_equal(o["kf"][:, 0] != 0, first != 0) and first.any() and not first.all()


def refresh_world(cases, after, seed=1200):
    """key-frame centres and the key-frame descriptor slab behind the observation records of append_cases()"""
    rng = np.random.default_rng(seed)
    kf = np.zeros(len(cases) + 1, KEYFRAME_CENTER_DTYPE)
    kf["left"][0] = cases[0]["P"]["cam1"]["Ow"]
    for b, c in enumerate(cases):
        kf["left"][b + 1] = c["P"]["cam2"]["Ow"]
    return kf, rng.integers(0, 256, (300 * (len(cases) + 1), 32), dtype=np.uint8)


def refreshed(after, kf, kf_desc, mp_desc, cap_mp):
    """the restated ComputeDistinctiveDescriptors / UpdateNormalAndDepth (tests/test_map_refresh.py) of the appended two-observation points"""
    n = int(after["n_mp"][0])
    start = after["obs_start"]
    points = [[tuple(int(v) for v in after["obs"][o]) for o in range(start[p], start[p + 1])] if p < n else [] for p in range(cap_mp)]
    S = Scene(after["mp"], mp_desc, points, after["ref"], kf, kf_desc, SF)
    return refresh_expected(S, REFRESH_DESCRIPTOR | REFRESH_NORMAL_DEPTH, sel=[int(p) for p in after["sel"]])


@pytest.mark.parametrize("backend", BACKENDS)
def test_append_then_refresh(lib, backend):
    """orbm_refresh_map_points(d_sel, n_sel = cap_sel) right behind the append == the restated two-observation refresh"""
    cases, created = append_cases()
    for c in cases[1:]:                                                  # one current key frame: every pair's first camera centre is the same
        c["P"]["cam1"]["Ow"] = cases[0]["P"]["cam1"]["Ow"]
    before, after = append_world(cases, created, **APPEND_ROOMY)
    before["mp"]["flags"][37:] = 0                                       # slots behind the cursor hold no point
    after["mp"]["flags"][int(after["n_mp"][0]):] = 0
    m, D_, out = run_append(lib, backend, cases, before, 400)
    kf, kf_desc = refresh_world(cases, after)
    mp_desc = np.full((400, 32), SENTINEL, np.uint8)
    d_desc = to_dev_plain(mp_desc.copy(), backend)
    res = m.RefreshMapPoints(D_["mp"], d_desc, D_["obs_start"], D_["obs"], D_["ref"], to_dev(kf, backend), to_dev_plain(kf_desc, backend),
                             m.RefreshParams(SF), sel=out["sel"])
    if backend == "hip":
        import torch
        torch.cuda.synchronize()
    mp_e, desc_e, best_e, st_e = refreshed(after, kf, kf_desc, mp_desc, 400)
    new = slice(37, int(after["n_mp"][0]))
    assert np.array_equal(nbits(to_host(D_["mp"]).reshape(-1).view(MAP_POINT_DTYPE)), nbits(mp_e)) and np.array_equal(to_host(d_desc), desc_e)
    assert np.array_equal(to_host(res["best_obs"])[new], best_e[new]) and np.array_equal(to_host(res["status"])[new], st_e[new])
    assert (st_e[new] == 3).all() and (best_e[new] == 0).all() and not np.array_equal(desc_e[new], mp_desc[new])


# ---------------------------------------------------------------------------------------------------- graph capture (GPU only)
@pytest.mark.gpu
def test_create_append_refresh_graph_replay_hip(hip_lib):
    """the linear create -> append -> refresh chain captured once on a single stream and replayed twice on changed inputs"""
    import torch
    cases, _ = append_cases()
    for c in cases[1:]:
        c["P"]["cam1"]["Ow"] = cases[0]["P"]["cam1"]["Ow"]
    s1, s2, pairs, m12 = batch_arrays(cases)
    m = orbhip.ORBmatcher(lib=hip_lib)
    d1, d2, dp, dm = upload_side(s1, "hip"), upload_side(s2, "hip"), to_dev(pairs, "hip"), to_dev_plain(m12, "hip")
    has0 = d1["has_mp"].clone(), d2["has_mp"].clone()
    kf, kf_desc = refresh_world(cases, None)
    d_kf, d_kfd = to_dev(kf, "hip"), to_dev_plain(kf_desc, "hip")
    mp_desc = np.full((400, 32), SENTINEL, np.uint8)
    prm = m.RefreshParams(SF)
    state = {}

    def world(m12_host):
        created = [restate_pair(pairs[b], host_side(s1, b), host_side(s2, b), m12_host[b], 120) for b in range(len(cases))]
        before, after = append_world(cases, created, **APPEND_ROOMY)
        before["mp"]["flags"][37:] = 0
        after["mp"]["flags"][int(after["n_mp"][0]):] = 0
        return created, before, after

    def chain():
        state["created"] = m.CreateNewMapPoints(d1, d2, dp, dm, 120, out=state.get("created"))
        m.AppendNewMapPoints(state["created"], dp, d1["kps"], state["n_mp"], state["mp"], 400, state["obs_start"], state["obs"], state["ref"], 300,
                             out=state["app"])
        state["res"] = m.RefreshMapPoints(state["mp"], state["desc"], state["obs_start"], state["obs"], state["ref"], d_kf, d_kfd, prm,
                                          sel=state["app"]["sel"], out=state.get("res"))

    def load(before):
        for k in ("mp", "obs", "ref"):
            t = to_dev(before[k], "hip")
            state[k] = t if k not in state else state[k].copy_(t)
        for k in ("obs_start", "n_mp"):
            t = to_dev_plain(before[k], "hip")
            state[k] = t if k not in state else state[k].copy_(t)
        t = to_dev_plain(mp_desc, "hip")
        state["desc"] = t if "desc" not in state else state["desc"].copy_(t)
        if "app" not in state:
            state["app"] = dict(sel=to_dev_plain(before["sel"].copy(), "hip"), appended=to_dev_plain(np.zeros(2, np.int32), "hip"))
        d1["has_mp"].copy_(has0[0])
        d2["has_mp"].copy_(has0[1])

    _, before, _ = world(m12)
    load(before)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain()                                                          # warm-up outside the capture: modules loaded, buffers allocated
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    verify_refreshed(state, m12, world, kf, kf_desc, mp_desc)
    counts = []
    load(before)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    rng = np.random.default_rng(1300)
    for it in range(2):
        m12_it = m12.copy()
        drop = rng.random(m12.shape) < 0.3
        m12_it[drop] = -1
        dm.copy_(to_dev_plain(m12_it, "hip"))
        _, before, _ = world(m12_it)
        load(before)
        torch.cuda.synchronize()
        g.replay()
        counts.append(verify_refreshed(state, m12_it, world, kf, kf_desc, mp_desc))
    assert counts[0] != counts[1] and min(counts) > 50


def verify_refreshed(state, m12_host, world, kf, kf_desc, mp_desc):
    """the graph's outputs against the restated create -> append -> refresh of the same inputs -> the number of points appended"""
    import torch
    torch.cuda.synchronize()
    _, _, after = world(m12_host)
    mp_e, desc_e, best_e, st_e = refreshed(after, kf, kf_desc, mp_desc, 400)
    new = slice(37, int(after["n_mp"][0]))
    assert list(to_host(state["app"]["appended"])) == list(after["appended"]) and int(to_host(state["n_mp"])[0]) == int(after["n_mp"][0])
    assert np.array_equal(to_host(state["app"]["sel"]), after["sel"]) and np.array_equal(to_host(state["obs_start"]), after["obs_start"])
    assert np.array_equal(to_host(state["obs"]).reshape(-1).view(np.int32), after["obs"].view(np.int32))
    assert np.array_equal(to_host(state["ref"]).reshape(-1).view(np.int32), after["ref"].view(np.int32))
    assert np.array_equal(nbits(to_host(state["mp"]).reshape(-1).view(MAP_POINT_DTYPE)), nbits(mp_e))
    assert np.array_equal(to_host(state["desc"]), desc_e)
    assert np.array_equal(to_host(state["res"]["status"])[new], st_e[new]) and np.array_equal(to_host(state["res"]["best_obs"])[new], best_e[new])
    return int(after["appended"][0])


# ---------------------------------------------------------------------------------------------------- coverage of the exits
def test_every_exit_is_reached():
    """every status code occurs in a batch that the tests above compare with the kernel (the restatements are shared through their keys)"""
    seen = set()
    for key, cases, cap_new in (("zoo", exit_zoo(), 200), ("w_zero", [w_zero_case()], 4), ("branch-ss", None, 150)):
        if cases is None:
            cases, key = [make_pair(400 + sum(map(ord, "ss")), 150, "ss", baseline=(0.5, 1.0))], ("branch", "ss")
        for e in restated(key, cases, cap_new):
            seen.update(int(c) for c in e["status"])
    c = make_pair(501, 120, "ss", baseline=(0.005, 0.01), depth=(0.6, 1.5), wrong=0.0)
    for S in (c["S1"], c["S2"]):
        S["kps_raw"] = S["kps"].copy()
        S["kps_raw"]["x"] += F(0.25)
    seen.update(int(v) for v in restated("stereo_unproject", [c], 120)[0]["status"])
    assert seen == set(range(15)), sorted(set(range(15)) - seen)
