// local_ba_host.h — the host halves of Optimizer::LocalBundleAdjustment restated serially over the flattened map (the records of
// include/orbhip.h "Local bundle adjustment on the device map"): the window selection and graph flattening (Optimizer.cc:1816-1945,
// :1978-2190, with the two guards of integration/Optimizer_hip.cc) and the outlier pass, erase loop and write-back (:2293-2510).  The
// yardstick of tests/cpp/local_ba_test.cpp and of tools/local_ba_timing.py; links no library.
#ifndef LOCAL_BA_HOST_H
#define LOCAL_BA_HOST_H
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <list>
#include <map>
#include <utility>
#include <vector>

#include "orbhip.h"
#include "orbslam3_hip/Optimizer.h"

namespace lba_host {

// The map as the device holds it, on the host
struct Map {
    std::vector<orbm_map_point> mp;
    std::vector<int32_t> obs_start;
    std::vector<orbm_observation> obs;
    std::vector<orbm_localmap_keyframe> kf;
    std::vector<int32_t> kf_mp;
    std::vector<orbm_cull_keyframe> ckf;
    std::vector<orbm_fusenb_pose> pose;
    std::vector<orbm_keyframe_center> center;
    std::vector<orbm_refresh_point> ref;
    std::vector<orb_keypoint> kps;
    std::vector<float> u_right;
    std::vector<int32_t> ordered_kf, n_ordered;   // [n_kf][cap_conn], [n_kf]
    std::vector<int32_t> nobs;                    // MapPoint::nObs
    std::vector<orbm_covis_keyframe> map;         // empty: one map
    int cap_conn = 1;
};

struct Window {
    std::vector<double> poses, points;
    std::vector<int32_t> hidx, lm_start, pose_start, pose_edges, pose_kf, pose_local, point_mp, edge_rec;
    std::vector<lba_edge> edges;
    uint32_t flags = 0;
    int n_local = 0, n_fixed = 0, num_fixed = 0, n_mono = 0, n_stereo = 0;
};

struct Applied {
    std::vector<std::pair<int, int>> erased;   // vToErase as (key frame, point)
    std::vector<int> went_bad;                 // in lLocalMapPoints order
    bool early = false;
    uint32_t flags = 0;
};

inline bool present(const Map& M, int k) { return k >= 0 && k < (int)M.kf.size() && (M.kf[k].flags & ORBM_LM_KF_PRESENT); }
inline bool same_map(const Map& M, int k, int cur) { return M.map.empty() || M.map[k].map_id == M.map[cur].map_id; }
inline bool in_graph(const Map& M, int k, int cur) { return !(M.kf[k].flags & ORBM_LM_KF_BAD) && same_map(M, k, cur); }

// the record check of the map-side calls -> the d_kf_mp row of the record's feature, or -1 (flagged)
inline int record_row(const Map& M, const orbm_observation& r, uint32_t* flags) {
    if (r.flags & ORBM_OBS_RIGHT) { *flags |= ORBM_LBA_UNSUPPORTED; return -1; }
    if (!present(M, r.kf)) { *flags |= ORBM_LBA_BAD_INDEX; return -1; }
    const long long i = (long long)r.desc_row - M.ckf[r.kf].desc_row0;
    if (i < 0 || i >= M.kf[r.kf].n_feat) { *flags |= ORBM_LBA_BAD_INDEX; return -1; }
    return M.kf[r.kf].mp_row0 + (int)i;
}

inline Window build(const Map& M, int cur, uint32_t init_id, int nlevels, const float* inv_level_sigma2) {
    Window W;
    if (!present(M, cur)) { W.flags |= ORBM_LBA_BAD_INDEX; W.lm_start.assign(1, 0); W.pose_start.assign(1, 0); return W; }
    const int n_kf = (int)M.kf.size(), n_mp = (int)M.mp.size();
    // ---- Local KeyFrames (:1813-1829)
    std::vector<uint8_t> local_mark(n_kf, 0), fixed_mark(n_kf, 0);
    std::list<int> lLocalKeyFrames, lFixedCameras;
    lLocalKeyFrames.push_back(cur);
    local_mark[cur] = 1;
    for (int r = 0; r < M.n_ordered[cur]; r++) {
        const int k = M.ordered_kf[(size_t)cur * M.cap_conn + r];
        if (!present(M, k)) { W.flags |= ORBM_LBA_BAD_INDEX; continue; }
        if (local_mark[k]) continue;
        local_mark[k] = 1;
        if (in_graph(M, k, cur)) lLocalKeyFrames.push_back(k);
    }
    // ---- Local MapPoints (:1831-1862)
    int num_fixedKF = 0;
    std::vector<uint8_t> point_mark(n_mp, 0);
    std::vector<int> lLocalMapPoints;
    for (int k : lLocalKeyFrames) {
        if (M.ckf[k].id == init_id) num_fixedKF = 1;
        for (int i = 0; i < M.kf[k].n_feat; i++) {
            const int p = M.kf_mp[M.kf[k].mp_row0 + i];
            if (p == -1) continue;
            if (p < 0 || p >= n_mp || !(M.mp[p].flags & ORBM_MP_VALID)) { W.flags |= ORBM_LBA_BAD_INDEX; continue; }
            if ((M.mp[p].flags & ORBM_MP_BAD) || point_mark[p]) continue;
            point_mark[p] = 1;
            lLocalMapPoints.push_back(p);
        }
    }
    // ---- Fixed Keyframes (:1864-1882)
    for (int p : lLocalMapPoints)
        for (int o = M.obs_start[p]; o < M.obs_start[p + 1]; o++) {
            const orbm_observation& r = M.obs[o];
            if (record_row(M, r, &W.flags) < 0 || !in_graph(M, r.kf, cur)) continue;
            if (!local_mark[r.kf] && !fixed_mark[r.kf]) { fixed_mark[r.kf] = 1; lFixedCameras.push_back(r.kf); }
        }
    num_fixedKF += (int)lFixedCameras.size();
    if (num_fixedKF < 2) {   // :1885-1931
        int lowerId = (int)M.ckf[cur].id, secondLowerId = (int)M.ckf[cur].id, pLowerKf = -1, pSecondLowerKF = -1;
        for (int k : lLocalKeyFrames) {
            if (k == cur || M.ckf[k].id == init_id) continue;
            if ((int)M.ckf[k].id < lowerId) { lowerId = (int)M.ckf[k].id; pLowerKf = k; }
            else if ((int)M.ckf[k].id < secondLowerId) { secondLowerId = (int)M.ckf[k].id; pSecondLowerKF = k; }
        }
        if (pLowerKf >= 0) {
            lFixedCameras.push_back(pLowerKf);
            lLocalKeyFrames.remove(pLowerKf);
            num_fixedKF++;
            if (num_fixedKF < 2 && pSecondLowerKF >= 0) {
                lFixedCameras.push_back(pSecondLowerKF);
                lLocalKeyFrames.remove(pSecondLowerKF);
                num_fixedKF++;
            }
        }
    }
    W.n_local = (int)lLocalKeyFrames.size(); W.n_fixed = (int)lFixedCameras.size(); W.num_fixed = num_fixedKF;
    // ---- the graph (:1957-2190): vertices by (mnId, slot)
    std::map<std::pair<uint32_t, int>, bool> kfById;   // -> local
    for (int k : lLocalKeyFrames) kfById[std::make_pair(M.ckf[k].id, k)] = true;
    for (int k : lFixedCameras) kfById[std::make_pair(M.ckf[k].id, k)] = false;
    std::vector<int> poseIdx(n_kf, -1);
    int nfree = 0;
    for (const auto& kv : kfById) {
        const int k = kv.first.second;
        double p7[7];
        float Tcw[12];   // GetPose(): [Rcw | tcw]
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) Tcw[r * 4 + c] = M.pose[k].Rcw[r * 3 + c]; Tcw[r * 4 + 3] = M.pose[k].tcw[r]; }
        orbslam3_hip::LbaLinearizer::poseFromTcw(Tcw, 4, p7);
        poseIdx[k] = (int)W.hidx.size();
        W.poses.insert(W.poses.end(), p7, p7 + 7);
        const bool fixed = !kv.second || M.ckf[k].id == init_id;
        W.hidx.push_back(fixed ? -1 : nfree++);
        W.pose_kf.push_back(k);
        W.pose_local.push_back(kv.second ? 1 : 0);
    }
    for (int p : lLocalMapPoints) {
        const int l = (int)W.point_mp.size();
        W.point_mp.push_back(p);
        for (int i = 0; i < 3; i++) W.points.push_back((double)M.mp[p].pos[i]);
        W.lm_start.push_back((int)W.edges.size());
        for (int o = M.obs_start[p]; o < M.obs_start[p + 1]; o++) {
            const orbm_observation& r = M.obs[o];
            uint32_t ignore = 0;
            const int row = record_row(M, r, &ignore);
            if (row < 0 || !in_graph(M, r.kf, cur)) continue;
            const orb_keypoint& kp = M.kps[row];
            if (kp.octave < 0 || kp.octave >= nlevels) { W.flags |= ORBM_LBA_BAD_INDEX; continue; }
            const float ur = M.u_right[row];
            const bool mono = ur < 0;
            lba_edge e{poseIdx[r.kf], l, (int16_t)(mono ? LBA_EDGE_MONO : LBA_EDGE_STEREO), 0, {kp.x, kp.y, mono ? 0.f : ur}, inv_level_sigma2[kp.octave]};
            W.edges.push_back(e);
            W.edge_rec.push_back(o);
            (mono ? W.n_mono : W.n_stereo)++;
        }
    }
    W.lm_start.push_back((int)W.edges.size());
    // BlockSolver::buildStructure: the per-pose edge lists, ascending
    const int np = (int)W.hidx.size(), ne = (int)W.edges.size();
    W.pose_start.assign(np + 1, 0);
    for (const lba_edge& e : W.edges) W.pose_start[e.pose + 1]++;
    for (int i = 0; i < np; i++) W.pose_start[i + 1] += W.pose_start[i];
    std::vector<int> fill(W.pose_start.begin(), W.pose_start.end() - 1);
    W.pose_edges.resize(ne);
    for (int i = 0; i < ne; i++) W.pose_edges[fill[W.edges[i].pose]++] = i;
    return W;
}

inline float norm3(const float* d) {   // cv::norm: sqrt of the double dot product
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)d[k] * (double)d[k];
    return (float)std::sqrt(s);
}

// Converter::toCvMat(SE3Quat) -> SetPose: Rcw | tcw as floats of to_homogeneous_matrix in double; Ow = -Rwc * tcw by one cv::gemm
inline void write_pose(const double* p7, orbm_fusenb_pose& T, orbm_keyframe_center& C) {
    const double x = p7[3], y = p7[4], z = p7[5], w = p7[6];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                         2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 9; i++) T.Rcw[i] = (float)R[i];
    for (int i = 0; i < 3; i++) T.tcw[i] = (float)p7[i];
    for (int r = 0; r < 3; r++) {
        double s = (double)T.Rcw[r] * (double)T.tcw[0];
        s += (double)T.Rcw[3 + r] * (double)T.tcw[1];
        s += (double)T.Rcw[6 + r] * (double)T.tcw[2];
        T.Ow[r] = C.left[r] = (float)(s * -1.0);
    }
}

// W: the window with the optimised poses / points.  M.nobs is MapPoint::nObs
inline Applied apply(Map& M, const Window& W, const double* chi2, const double* depth, const float* sf, int nlevels) {
    Applied A;
    const int ne = (int)W.edges.size(), nl = (int)W.point_mp.size(), n_mp = (int)M.mp.size();
    // ---- outlier edges (:2293-2344): mono, then stereo
    std::vector<int> vToErase;   // edge indices
    for (int pass = 0; pass < 2; pass++)
        for (int e = 0; e < ne; e++) {
            const bool mono = W.edges[e].kind == LBA_EDGE_MONO;
            if (mono != (pass == 0)) continue;
            if (chi2[e] > (mono ? 5.991 : 7.815) || !(depth[e] > 0.0)) vToErase.push_back(e);
        }
    for (int e : vToErase) A.erased.emplace_back(W.pose_kf[W.edges[e].pose], W.point_mp[W.edges[e].point]);
    if ((double)vToErase.size() >= (double)ne * 0.5) { A.early = true; return A; }
    // ---- the erase loop (:2390-2401) with EraseObservation and SetBadFlag
    std::vector<uint8_t> dead(M.obs.size(), 0), bad_now(n_mp, 0);
    const std::vector<orbm_refresh_point> ref0 = M.ref;
    for (int e : vToErase) {
        const int p = W.point_mp[W.edges[e].point], o = W.edge_rec[e];
        if (bad_now[p] || dead[o]) continue;
        const int s = M.obs_start[p], en = M.obs_start[p + 1];
        const int row = record_row(M, M.obs[o], &A.flags);
        if (row < 0) continue;
        M.kf_mp[row] = -1;
        dead[o] = 1;
        M.nobs[p] -= M.u_right[row] >= 0 ? 2 : 1;
        const bool ref_died = M.obs[o].kf == M.ref[p].ref_kf;
        if (M.nobs[p] <= 2) {
            bad_now[p] = 1;
            M.mp[p].flags |= ORBM_MP_BAD;
            M.ref[p] = ref0[p];   // (a bad point keeps its entry: the rule of orbm_cull_apply.d_ref)
            for (int o2 = s; o2 < en; o2++) {
                if (dead[o2]) continue;
                uint32_t ignore = 0;
                const int row2 = record_row(M, M.obs[o2], &ignore);
                if (row2 >= 0) M.kf_mp[row2] = -1;
                dead[o2] = 1;
            }
        } else if (ref_died) {
            for (int o2 = s; o2 < en; o2++) {
                uint32_t ignore = 0;
                const int row2 = dead[o2] ? -1 : record_row(M, M.obs[o2], &ignore);
                if (row2 < 0) continue;
                M.ref[p].ref_kf = M.obs[o2].kf;
                M.ref[p].level = M.kps[row2].octave;
                break;
            }
        }
        M.mp[p].flags = (M.mp[p].flags & ~ORBM_MP_HAS_OBS) | (M.nobs[p] > 0 ? ORBM_MP_HAS_OBS : 0u);
    }
    for (int l = 0; l < nl; l++)
        if (bad_now[W.point_mp[l]]) A.went_bad.push_back(W.point_mp[l]);
    // the surviving rows
    std::vector<orbm_observation> obs;
    std::vector<int32_t> start(n_mp + 1, 0);
    for (int p = 0; p < n_mp; p++) {
        start[p] = (int)obs.size();
        if (!(M.mp[p].flags & ORBM_MP_VALID)) continue;
        for (int o = M.obs_start[p]; o < M.obs_start[p + 1]; o++)
            if (!dead[o]) obs.push_back(M.obs[o]);
    }
    start[n_mp] = (int)obs.size();
    M.obs.swap(obs);
    M.obs_start.swap(start);
    // ---- Recover optimized data: key frames (:2425-2433), then points (:2499-2506)
    for (size_t i = 0; i < W.pose_kf.size(); i++)
        if (W.pose_local[i]) write_pose(&W.poses[7 * i], M.pose[W.pose_kf[i]], M.center[W.pose_kf[i]]);
    for (int l = 0; l < nl; l++) {
        const int p = W.point_mp[l];
        orbm_map_point& m = M.mp[p];
        for (int i = 0; i < 3; i++) m.pos[i] = (float)W.points[3 * l + i];
        const int s = M.obs_start[p], en = M.obs_start[p + 1];
        if ((m.flags & ORBM_MP_BAD) || en == s) continue;   // UpdateNormalAndDepth
        float normal[3] = {0, 0, 0};
        for (int o = s; o < en; o++) {
            float d[3];
            for (int k = 0; k < 3; k++) d[k] = m.pos[k] - M.center[M.obs[o].kf].left[k];
            const float nr = norm3(d);
            for (int k = 0; k < 3; k++) normal[k] = normal[k] + d[k] / nr;
        }
        float PC[3];
        for (int k = 0; k < 3; k++) PC[k] = m.pos[k] - M.center[M.ref[p].ref_kf].left[k];
        const float dist = norm3(PC);
        m.max_distance = dist * sf[M.ref[p].level];
        m.min_distance = m.max_distance / sf[nlevels - 1];
        for (int k = 0; k < 3; k++) m.normal[k] = normal[k] / (float)(en - s);
    }
    return A;
}

}  // namespace lba_host
#endif
