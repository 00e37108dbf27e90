// new_map_points_host.h — the loop a caller runs on the host today behind SearchForTriangulation: LocalMapping::CreateNewMapPoints
// (LocalMapping.cc:651-904) for one (current key frame, neighbour) pair over flattened arrays, with the arithmetic of rule R6 (DESIGN.md
// section 2).  tests/cpp/new_map_points_test.cpp compares the device path with it; tools/new_points_timing.py times it (compiled -O3
// -ffp-contract=off) as the baseline of the device chain.  Host code only.
#ifndef NEW_MAP_POINTS_HOST_H
#define NEW_MAP_POINTS_HOST_H
#include <cmath>
#include <cstdint>
#include <vector>

#include <orbhip.h>

namespace newpt_host {

inline float gemm3(float a0, float a1, float a2, const float* x, double c) {
    double s = 0.0;
    s += (double)a0 * (double)x[0];
    s += (double)a1 * (double)x[1];
    s += (double)a2 * (double)x[2];
    return (float)(s + c);
}
inline double ddot3(const float* a, const float* b) {
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += (double)a[k] * (double)b[k];
    return s;
}
inline void kb8_unproject(const float* p, float u, float v, float* ray) {   // KannalaBrandt8.cpp:101-124, rule R4
    const float pwx = (u - p[2]) / p[0], pwy = (v - p[3]) / p[1];
    float scale = 1.f;
    float theta_d = sqrtf(pwx * pwx + pwy * pwy);
    theta_d = fminf(fmaxf(-(float)(3.14159265358979323846 / 2.0), theta_d), (float)(3.14159265358979323846 / 2.0));
    if (theta_d > 1e-8) {
        float theta = theta_d;
        for (int j = 0; j < 10; j++) {
            const float t2 = theta * theta, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
            const float k0 = p[4] * t2, k1 = p[5] * t4, k2 = p[6] * t6, k3 = p[7] * t8;
            const float fix = (theta * (1 + k0 + k1 + k2 + k3) - theta_d) / (1 + 3 * k0 + 5 * k1 + 7 * k2 + 9 * k3);
            theta = theta - fix;
            if (fabsf(fix) < 1e-6f) break;
        }
        scale = (float)tan((double)theta) / theta_d;
    }
    ray[0] = pwx * scale; ray[1] = pwy * scale; ray[2] = 1.f;
}
inline void kb8_project(const float* p, const float* X, float* uv) {   // KannalaBrandt8.cpp:28-42, rule R4
    const float x2y2 = X[0] * X[0] + X[1] * X[1];
    const float theta = (float)atan2((double)sqrtf(x2y2), (double)X[2]);
    const float psi = (float)atan2((double)X[1], (double)X[0]);
    const float t2 = theta * theta, t3 = theta * t2, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
    const float r = theta + p[4] * t3 + p[5] * t5 + p[6] * t7 + p[7] * t9;
    uv[0] = (float)((double)(p[0] * r) * cos((double)psi) + (double)p[2]);
    uv[1] = (float)((double)(p[1] * r) * sin((double)psi) + (double)p[3]);
}
inline void unproject(const orbm_newpt_camera& c, float u, float v, float* xn) {
    if (c.camera_type == ORBM_CAM_KB8) { kb8_unproject(c.k, u, v, xn); return; }
    xn[0] = (u - c.k[2]) / c.k[0]; xn[1] = (v - c.k[3]) / c.k[1]; xn[2] = 1.f;
}
inline void project(const orbm_newpt_camera& c, const float* X, float* uv) {
    if (c.camera_type == ORBM_CAM_KB8) { kb8_project(c.k, X, uv); return; }
    uv[0] = c.k[0] * X[0] / X[2] + c.k[2]; uv[1] = c.k[1] * X[1] / X[2] + c.k[3];
}
// the last row of cv::SVD's vt as rule R4 states it: cyclic Jacobi on A^T A in double, 8 sweeps, the first least diagonal entry
inline void null_vector4(const float* A, float* v4) {
    double M[16], V[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += (double)A[k * 4 + i] * (double)A[k * 4 + j];
            M[i * 4 + j] = s; V[i * 4 + j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 8; sweep++)
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                const double apq = M[p * 4 + q];
                if (apq == 0.0) continue;
                const double th = (M[q * 4 + q] - M[p * 4 + p]) / (2.0 * apq);
                const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < 4; k++) { const double a = M[k * 4 + p], b = M[k * 4 + q]; M[k * 4 + p] = c * a - sn * b; M[k * 4 + q] = sn * a + c * b; }
                for (int k = 0; k < 4; k++) { const double a = M[p * 4 + k], b = M[q * 4 + k]; M[p * 4 + k] = c * a - sn * b; M[q * 4 + k] = sn * a + c * b; }
                for (int k = 0; k < 4; k++) { const double a = V[k * 4 + p], b = V[k * 4 + q]; V[k * 4 + p] = c * a - sn * b; V[k * 4 + q] = sn * a + c * b; }
            }
    int m = 0;
    for (int i = 1; i < 4; i++) if (M[i * 4 + i] < M[m * 4 + m]) m = i;
    for (int k = 0; k < 4; k++) v4[k] = (float)V[k * 4 + m];
}
inline float stereo_cos(float mb, float depth) {
    const float th = (float)atan2((double)(mb / 2.f), (double)depth);
    const float a = 2.f * th;
    return (float)cos((double)a);
}
inline bool unproject_stereo(const orbm_newpt_camera& c, const orb_keypoint& raw, float z, float* x3D) {
    if (!(z > 0)) return false;
    const float xc[3] = {(raw.x - c.k[2]) * z * c.invfx, (raw.y - c.k[3]) * z * c.invfy, z};
    for (int i = 0; i < 3; i++) x3D[i] = gemm3(c.Rcw[i], c.Rcw[3 + i], c.Rcw[6 + i], xc, (double)c.Ow[i]);
    return true;
}
inline bool reproj_rejects(const orbm_newpt_camera& c, float mbf, const float* x3D, float z, const orb_keypoint& kp, bool stereo, float ur, float sigma2) {
    float P[3] = {gemm3(c.Rcw[0], c.Rcw[1], c.Rcw[2], x3D, (double)c.tcw[0]), gemm3(c.Rcw[3], c.Rcw[4], c.Rcw[5], x3D, (double)c.tcw[1]), z};
    const float invz = (float)(1.0 / (double)z);
    if (!stereo) {
        float uv[2];
        project(c, P, uv);
        const float ex = uv[0] - kp.x, ey = uv[1] - kp.y;
        return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
    }
    const float u = c.k[0] * P[0] * invz + c.k[2];
    const float u_r = u - mbf * invz;
    const float v = c.k[1] * P[1] * invz + c.k[3];
    const float ex = u - kp.x, ey = v - kp.y, er = u_r - ur;
    return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}
inline float dist_to(const float* x3D, const float* Ow) {
    const float d[3] = {x3D[0] - Ow[0], x3D[1] - Ow[1], x3D[2] - Ow[2]};
    return (float)sqrt(ddot3(d, d));
}

struct Side {
    const orb_keypoint* kps; const orb_keypoint* kps_raw; const float* u_right; const float* depth;
};

// one match -> ORBM_NEWPT_* exit code (LocalMapping.cc:653-904)
inline int create_one(const orbm_newpt_pair& P, const Side& S1, const Side& S2, int i1, int i2, float* x3D) {
    const orbm_newpt_camera& c1 = P.cam1;
    const orbm_newpt_camera& c2 = P.cam2;
    const orb_keypoint& kp1 = S1.kps[i1];
    const orb_keypoint& kp2 = S2.kps[i2];
    if (kp1.octave < 0 || kp1.octave >= 16 || kp2.octave < 0 || kp2.octave >= 16) return ORBM_NEWPT_BAD_INDEX;
    const float ur1 = S1.u_right ? S1.u_right[i1] : -1.f, ur2 = S2.u_right ? S2.u_right[i2] : -1.f;
    const bool st1 = ur1 >= 0, st2 = ur2 >= 0;
    float xn1[3], xn2[3], ray1[3], ray2[3];
    unproject(c1, kp1.x, kp1.y, xn1);
    unproject(c2, kp2.x, kp2.y, xn2);
    for (int i = 0; i < 3; i++) {
        ray1[i] = gemm3(c1.Rcw[i], c1.Rcw[3 + i], c1.Rcw[6 + i], xn1, 0.0);
        ray2[i] = gemm3(c2.Rcw[i], c2.Rcw[3 + i], c2.Rcw[6 + i], xn2, 0.0);
    }
    const float cosRays = (float)(ddot3(ray1, ray2) / (sqrt(ddot3(ray1, ray1)) * sqrt(ddot3(ray2, ray2))));
    float cs1 = cosRays + 1, cs2 = cosRays + 1;
    if (st1) cs1 = stereo_cos(c1.mb, S1.depth[i1]);
    else if (st2) cs2 = stereo_cos(c2.mb, S2.depth[i2]);
    const float cosStereo = cs2 < cs1 ? cs2 : cs1;
    int how;
    if (cosRays < cosStereo && cosRays > 0 && (st1 || st2 || (double)cosRays < 0.9998)) {
        float A[16];
        for (int c = 0; c < 4; c++) {
            const float T1r0 = c < 3 ? c1.Rcw[c] : c1.tcw[0], T1r1 = c < 3 ? c1.Rcw[3 + c] : c1.tcw[1], T1r2 = c < 3 ? c1.Rcw[6 + c] : c1.tcw[2];
            const float T2r0 = c < 3 ? c2.Rcw[c] : c2.tcw[0], T2r1 = c < 3 ? c2.Rcw[3 + c] : c2.tcw[1], T2r2 = c < 3 ? c2.Rcw[6 + c] : c2.tcw[2];
            A[c] = xn1[0] * T1r2 - T1r0;
            A[4 + c] = xn1[1] * T1r2 - T1r1;
            A[8 + c] = xn2[0] * T2r2 - T2r0;
            A[12 + c] = xn2[1] * T2r2 - T2r1;
        }
        float v4[4];
        null_vector4(A, v4);
        if (v4[3] == 0) return ORBM_NEWPT_W_ZERO;
        for (int i = 0; i < 3; i++) x3D[i] = v4[i] / v4[3];
        how = ORBM_NEWPT_CREATED_TRIANGULATED;
    } else if (st1 && cs1 < cs2) {
        if (!unproject_stereo(c1, (S1.kps_raw ? S1.kps_raw : S1.kps)[i1], S1.depth[i1], x3D)) return ORBM_NEWPT_EMPTY_STEREO;
        how = ORBM_NEWPT_CREATED_STEREO1;
    } else if (st2 && cs2 < cs1) {
        if (!unproject_stereo(c2, (S2.kps_raw ? S2.kps_raw : S2.kps)[i2], S2.depth[i2], x3D)) return ORBM_NEWPT_EMPTY_STEREO;
        how = ORBM_NEWPT_CREATED_STEREO2;
    } else {
        return ORBM_NEWPT_LOW_PARALLAX;
    }
    const float z1 = gemm3(c1.Rcw[6], c1.Rcw[7], c1.Rcw[8], x3D, (double)c1.tcw[2]);
    if (z1 <= 0) return ORBM_NEWPT_BEHIND_1;
    const float z2 = gemm3(c2.Rcw[6], c2.Rcw[7], c2.Rcw[8], x3D, (double)c2.tcw[2]);
    if (z2 <= 0) return ORBM_NEWPT_BEHIND_2;
    if (reproj_rejects(c1, c1.mbf, x3D, z1, kp1, st1, ur1, c1.level_sigma2[kp1.octave])) return ORBM_NEWPT_REPROJ_1;
    if (reproj_rejects(c2, c1.mbf, x3D, z2, kp2, st2, ur2, c2.level_sigma2[kp2.octave])) return ORBM_NEWPT_REPROJ_2;
    const float d1 = dist_to(x3D, c1.Ow), d2 = dist_to(x3D, c2.Ow);
    if (d1 == 0 || d2 == 0) return ORBM_NEWPT_ZERO_DIST;
    if (P.far_points && (d1 >= P.th_far_points || d2 >= P.th_far_points)) return ORBM_NEWPT_FAR;
    const float ratioDist = d2 / d1;
    const float ratioOctave = c1.scale_factors[kp1.octave] / c2.scale_factors[kp2.octave];
    if (ratioDist * P.ratio_factor < ratioOctave || ratioDist > ratioOctave * P.ratio_factor) return ORBM_NEWPT_SCALE;
    return how;
}

// the loop over match12 [n1] (idx2 or -1): appends the created points and marks has_mp1 / has_mp2; returns their number
inline int create_loop(const orbm_newpt_pair& P, const Side& S1, const Side& S2, const int32_t* match12, int n1, uint8_t* has_mp1, uint8_t* has_mp2,
                       std::vector<orbm_new_point>& out) {
    int created = 0;
    for (int i1 = 0; i1 < n1; i1++) {
        const int i2 = match12[i1];
        if (i2 < 0) continue;
        orbm_new_point np;
        const int code = create_one(P, S1, S2, i1, i2, np.pos);
        if (code < ORBM_NEWPT_CREATED_TRIANGULATED || code > ORBM_NEWPT_CREATED_STEREO2) continue;
        np.idx1 = i1; np.idx2 = i2; np.how = code;
        out.push_back(np);
        if (has_mp1) has_mp1[i1] = 1;
        if (has_mp2) has_mp2[i2] = 1;
        created++;
    }
    return created;
}

}  // namespace newpt_host
#endif
