// local_ba_synth.h — a synthetic map for the local bundle adjustment (tests/cpp/local_ba_test.cpp, tools/local_ba_timing.py): key frames on a
// circle of radius 10 looking inward at a box of points, real pinhole projections with octave noise and a few gross outliers, 40 % stereo
// features.  Slots [0, n_fixed) hold key frames that are not covisible with the current one (the last slot); every other is.  A feature
// whose point has one view holds no point (one view does not constrain it).  DeviceMap puts such a map on the device as an adapter's caller
// would hold it.
#ifndef LOCAL_BA_SYNTH_H
#define LOCAL_BA_SYNTH_H
#include <random>

#include "local_ba_host.h"

namespace lba_synth {

struct World {
    lba_host::Map M;
    int current = 0, nlevels = 8;
    uint32_t init_id = 0;
    float sf[16], inv_sigma2[16];
    lba_camera cam;
};

inline World make(unsigned seed, int n_kf, int n_feat, int n_mp, int n_fixed, int fixed_feat = 100) {
    const double FX = 458.654, FY = 457.296, CX = 367.215, CY = 248.375, BF = 47.906;
    World W;
    std::memset(&W.cam, 0, sizeof W.cam);
    W.cam.model = LBA_CAM_PINHOLE;
    W.cam.p[0] = (float)FX; W.cam.p[1] = (float)FY; W.cam.p[2] = (float)CX; W.cam.p[3] = (float)CY; W.cam.bf = (float)BF; W.cam.trl_q[3] = 1.0;
    W.sf[0] = 1.f;
    for (int i = 1; i < 16; i++) W.sf[i] = W.sf[i - 1] * 1.2f;
    for (int i = 0; i < 16; i++) W.inv_sigma2[i] = 1.f / (W.sf[i] * W.sf[i]);
    std::mt19937 g(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    lba_host::Map& M = W.M;
    const int n_all = n_kf + n_fixed;
    std::vector<float> pts((size_t)n_mp * 3);
    for (int p = 0; p < n_mp; p++) { pts[3 * p] = (float)(8 * U(g) - 4); pts[3 * p + 1] = (float)(8 * U(g) - 4); pts[3 * p + 2] = (float)(3 * U(g) - 1.5); }
    std::vector<int> views(n_mp, 0);
    for (int k = 0; k < n_all; k++) {
        const double a = 2 * M_PI * k / n_all;
        double c[3] = {10 * std::cos(a), 10 * std::sin(a), 0.2 * N(g)}, z[3], x[3], y[3];
        double nz = 0;
        for (int i = 0; i < 3; i++) { z[i] = -c[i] / std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) + 0.02 * N(g); }
        for (int i = 0; i < 3; i++) nz += z[i] * z[i];
        for (int i = 0; i < 3; i++) z[i] /= std::sqrt(nz);
        x[0] = -z[1]; x[1] = z[0]; x[2] = 0;   // (0, 0, 1) x z
        const double nx = std::sqrt(x[0] * x[0] + x[1] * x[1]);
        for (int i = 0; i < 3; i++) x[i] /= nx;
        y[0] = z[1] * x[2] - z[2] * x[1]; y[1] = z[2] * x[0] - z[0] * x[2]; y[2] = z[0] * x[1] - z[1] * x[0];
        orbm_fusenb_pose T;
        std::memset(&T, 0, sizeof T);
        for (int i = 0; i < 3; i++) { T.Rcw[i] = (float)x[i]; T.Rcw[3 + i] = (float)y[i]; T.Rcw[6 + i] = (float)z[i]; }
        for (int r = 0; r < 3; r++) T.tcw[r] = (float)-((double)T.Rcw[3 * r] * c[0] + (double)T.Rcw[3 * r + 1] * c[1] + (double)T.Rcw[3 * r + 2] * c[2]);
        orbm_localmap_keyframe K;
        std::memset(&K, 0, sizeof K);
        K.flags = ORBM_LM_KF_PRESENT; K.parent = K.prev = -1; K.mp_row0 = (int)M.kf_mp.size();
        for (int i = 0; i < 10; i++) K.covis[i] = -1;
        const int want = k < n_fixed ? fixed_feat : n_feat;
        // the visible points, then a random choice of `want` of them in index order (selection sampling)
        std::vector<int> vis;
        std::vector<double> uu(n_mp), vv(n_mp), zz(n_mp);
        for (int p = 0; p < n_mp; p++) {
            double Xc[3];
            for (int r = 0; r < 3; r++) Xc[r] = (double)T.Rcw[3 * r] * pts[3 * p] + (double)T.Rcw[3 * r + 1] * pts[3 * p + 1] + (double)T.Rcw[3 * r + 2] * pts[3 * p + 2] + (double)T.tcw[r];
            uu[p] = FX * Xc[0] / Xc[2] + CX; vv[p] = FY * Xc[1] / Xc[2] + CY; zz[p] = Xc[2];
            if (Xc[2] > 0.5 && uu[p] > 0 && uu[p] < 752 && vv[p] > 0 && vv[p] < 480) vis.push_back(p);
        }
        int left = (int)vis.size(), need = want < left ? want : left;
        for (int p : vis) {
            if (need > 0 && U(g) * left < need) {
                const int oct = (int)(U(g) * W.nlevels) % W.nlevels;
                const double s = 0.7 * W.sf[oct];
                double du = s * N(g), dv = s * N(g), dr = s * N(g);
                if (U(g) < 0.03) { du = 30 * N(g); dv = 30 * N(g); }
                orb_keypoint kp;
                std::memset(&kp, 0, sizeof kp);
                kp.x = (float)(uu[p] + du); kp.y = (float)(vv[p] + dv); kp.size = 31.f; kp.octave = oct;
                M.kps.push_back(kp);
                M.u_right.push_back(U(g) < 0.4 ? (float)(uu[p] + du - BF / zz[p] + dr) : -1.f);
                M.kf_mp.push_back(p);
                views[p]++;
                need--;
            }
            left--;
        }
        K.n_feat = (int)M.kf_mp.size() - K.mp_row0;
        if (k >= n_fixed + 2)   // the free poses start off the truth
            for (int r = 0; r < 3; r++) T.tcw[r] = (float)(T.tcw[r] + 0.01 * N(g));
        orbm_keyframe_center C;
        std::memset(&C, 0, sizeof C);
        for (int r = 0; r < 3; r++) T.Ow[r] = C.left[r] = (float)-((double)T.Rcw[r] * T.tcw[0] + (double)T.Rcw[3 + r] * T.tcw[1] + (double)T.Rcw[6 + r] * T.tcw[2]);
        orbm_cull_keyframe ck;
        std::memset(&ck, 0, sizeof ck);
        ck.id = 10u + (uint32_t)k; ck.prev = ck.next = -1; ck.desc_row0 = K.mp_row0;
        M.kf.push_back(K); M.ckf.push_back(ck); M.pose.push_back(T); M.center.push_back(C);
    }
    for (int32_t& p : M.kf_mp)
        if (views[p] < 2) p = -1;
    // the records: per point by key-frame slot (= pointer rank here)
    std::vector<std::vector<orbm_observation>> rows(n_mp);
    for (int k = 0; k < n_all; k++)
        for (int i = 0; i < M.kf[k].n_feat; i++) {
            const int p = M.kf_mp[M.kf[k].mp_row0 + i];
            if (p >= 0) rows[p].push_back(orbm_observation{k, M.ckf[k].desc_row0 + i, 0u});
        }
    M.obs_start.assign(1, 0);
    for (int p = 0; p < n_mp; p++) {
        orbm_map_point m;
        std::memset(&m, 0, sizeof m);
        for (int i = 0; i < 3; i++) m.pos[i] = (float)(pts[3 * p + i] + 0.02 * N(g));
        m.normal[2] = 1.f; m.min_distance = 1.f; m.max_distance = 20.f; m.desc_row = p;
        int nobs = 0;
        for (const orbm_observation& r : rows[p]) { M.obs.push_back(r); nobs += M.u_right[M.kf[r.kf].mp_row0 + r.desc_row - M.ckf[r.kf].desc_row0] >= 0 ? 2 : 1; }
        m.flags = ORBM_MP_VALID | (nobs > 0 ? ORBM_MP_HAS_OBS : 0u);
        M.mp.push_back(m);
        M.nobs.push_back(nobs);
        M.obs_start.push_back((int)M.obs.size());
        orbm_refresh_point rf{0, 0};
        if (!rows[p].empty()) { rf.ref_kf = rows[p][0].kf; rf.level = M.kps[M.kf[rf.ref_kf].mp_row0 + rows[p][0].desc_row - M.ckf[rf.ref_kf].desc_row0].octave; }
        M.ref.push_back(rf);
    }
    M.cap_conn = n_kf;
    M.ordered_kf.assign((size_t)n_all * M.cap_conn, -1);
    M.n_ordered.assign(n_all, 0);
    W.current = n_all - 1;
    for (int r = 0; r < n_kf - 1; r++) M.ordered_kf[(size_t)W.current * M.cap_conn + r] = n_all - 2 - r;
    M.n_ordered[W.current] = n_kf - 1;
    W.init_id = 10u + (uint32_t)n_fixed;
    return W;
}

// device -> host, synchronised
template <class T> std::vector<T> fetch(const T* d, size_t n) {
    std::vector<T> h(n);
    if (n) orbslam3_hip::detail::download(h.data(), d, n * sizeof(T), nullptr);
    orbslam3_hip::detail::check(orb_stream_sync(nullptr), "sync");
    return h;
}


// the map on the device: the slabs the adapter's caller owns
struct DeviceMap {
    orbslam3_hip::detail::DevBuf mp, start, obs, kf, kf_mp, ckf, pose, center, ref, kps, ur, ord, nord, nobs, start2, obs2;
    orbm_localmap_view V;
    orbm_lba_in I;
    orbm_lba_apply A;
    size_t n_obs = 0;
    void upload(const World& W) {
        const lba_host::Map& M = W.M;
        std::memset(&V, 0, sizeof V); std::memset(&I, 0, sizeof I); std::memset(&A, 0, sizeof A);
        V.d_mp = A.d_mp = mp.upload(M.mp.data(), M.mp.size());
        V.d_obs_start = start.upload(M.obs_start.data(), M.obs_start.size());
        V.d_obs = obs.upload(M.obs.data(), M.obs.size());
        V.d_kf = kf.upload(M.kf.data(), M.kf.size());
        V.d_kf_mp = A.d_kf_mp = kf_mp.upload(M.kf_mp.data(), M.kf_mp.size());
        V.n_mp = (int)M.mp.size(); V.n_obs = (int)M.obs.size(); V.n_kf = (int)M.kf.size(); V.n_kf_mp_rows = (int)M.kf_mp.size();
        I.d_ckf = ckf.upload(M.ckf.data(), M.ckf.size());
        I.d_pose = A.d_pose = pose.upload(M.pose.data(), M.pose.size());
        I.d_kps = kps.upload(M.kps.data(), M.kps.size());
        I.d_u_right = ur.upload(M.u_right.data(), M.u_right.size());
        I.d_ordered_kf = ord.upload(M.ordered_kf.data(), M.ordered_kf.size());
        I.d_n_ordered = nord.upload(M.n_ordered.data(), M.n_ordered.size());
        I.cap_conn = M.cap_conn; I.nlevels = W.nlevels;
        for (int i = 0; i < 16; i++) { I.inv_level_sigma2[i] = W.inv_sigma2[i]; I.scale_factors[i] = W.sf[i]; }
        A.d_center = center.upload(M.center.data(), M.center.size());
        A.d_ref = ref.upload(M.ref.data(), M.ref.size());
        A.d_mp_nobs = nobs.upload(M.nobs.data(), M.nobs.size());
        A.d_obs_start_out = (int32_t*)start2.ensure(M.obs_start.size() * 4 + 16);
        A.d_obs_out = (orbm_observation*)obs2.ensure(M.obs.size() * sizeof(orbm_observation) + 16);
        A.cap_obs_out = (int)M.obs.size();
        n_obs = M.obs.size();
    }
    // the map as the device holds it now (applied: the out-CSR is the CSR)
    lba_host::Map download(const lba_host::Map& like, bool applied, int n_obs_out) const {
        lba_host::Map M = like;
        M.mp = fetch(V.d_mp, like.mp.size());
        M.kf_mp = fetch(V.d_kf_mp, like.kf_mp.size());
        M.pose = fetch((const orbm_fusenb_pose*)A.d_pose, like.pose.size());
        M.center = fetch((const orbm_keyframe_center*)A.d_center, like.center.size());
        M.ref = fetch((const orbm_refresh_point*)A.d_ref, like.ref.size());
        M.nobs = fetch((const int32_t*)A.d_mp_nobs, like.nobs.size());
        if (applied) {
            M.obs_start = fetch((const int32_t*)A.d_obs_start_out, like.obs_start.size());
            M.obs = fetch((const orbm_observation*)A.d_obs_out, (size_t)n_obs_out);
        }
        return M;
    }
};

}  // namespace lba_synth
#endif
