// local_ba_host_test.cpp — the host restatement (local_ba_host.h) alone, on a hand-made map with a worked-out answer, and on a synthetic
// world whose invariants are checked; links no library, so it also runs under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstdio>
#include <cstdlib>

#include "local_ba_synth.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// a key frame with the identity rotation at tcw = (x, 0, 0) whose features hold `points` (mono, octave = the feature's index)
static void add_kf(lba_host::Map& M, uint32_t id, const std::vector<int>& points, float x, const std::vector<float>& ur = {}) {
    orbm_localmap_keyframe k;
    std::memset(&k, 0, sizeof k);
    k.flags = ORBM_LM_KF_PRESENT; k.parent = k.prev = -1; k.mp_row0 = (int)M.kf_mp.size(); k.n_feat = (int)points.size();
    orbm_cull_keyframe c;
    std::memset(&c, 0, sizeof c);
    c.id = id; c.prev = c.next = -1; c.desc_row0 = k.mp_row0;
    orbm_fusenb_pose T;
    std::memset(&T, 0, sizeof T);
    T.Rcw[0] = T.Rcw[4] = T.Rcw[8] = 1.f; T.tcw[0] = x; T.Ow[0] = -x;
    orbm_keyframe_center ce;
    std::memset(&ce, 0, sizeof ce);
    ce.left[0] = -x;
    for (size_t i = 0; i < points.size(); i++) {
        M.kf_mp.push_back(points[i]);
        orb_keypoint kp;
        std::memset(&kp, 0, sizeof kp);
        kp.x = 100.f * (float)M.kf.size() + (float)i; kp.y = 7.f; kp.octave = (int)i;
        M.kps.push_back(kp);
        M.u_right.push_back(i < ur.size() ? ur[i] : -1.f);
    }
    M.kf.push_back(k); M.ckf.push_back(c); M.pose.push_back(T); M.center.push_back(ce);
}

int main() {
    float sf[8] = {1.f}, inv[8];
    for (int i = 1; i < 8; i++) sf[i] = sf[i - 1] * 1.2f;
    for (int i = 0; i < 8; i++) inv[i] = 1.f / (sf[i] * sf[i]);
    {   // Slots 0, 1, 2 with ids 8, 9, 7.  The current key frame (slot 1) sees slot 0; slot 2 shares point 1 only: fixed.  One fixed is
        // fewer than two, so the branch moves the lowest local id that is not the current one's (8, slot 0) to the fixed ones.
        lba_host::Map M;
        add_kf(M, 8, {0, 1}, 1.f, {-1.f, 30.5f});
        add_kf(M, 9, {0, -1}, 2.f);
        add_kf(M, 7, {1}, 3.f);
        for (int p = 0; p < 2; p++) {
            orbm_map_point m;
            std::memset(&m, 0, sizeof m);
            m.pos[0] = (float)p; m.pos[2] = 4.f; m.flags = ORBM_MP_VALID | ORBM_MP_HAS_OBS;
            M.mp.push_back(m);
        }
        // rows in pointer order 1, 0, 2: point 0 = (kf 1, f 0), (kf 0, f 0); point 1 = (kf 0, f 1), (kf 2, f 0)
        M.obs = {{1, 2, 0u}, {0, 0, 0u}, {0, 1, 0u}, {2, 4, 0u}};
        M.obs_start = {0, 2, 4};
        M.nobs = {2, 3};
        M.ref = {{1, 0}, {0, 1}};
        M.cap_conn = 2;
        M.ordered_kf = {-1, -1, 0, -1, -1, -1};
        M.n_ordered = {0, 1, 0};
        const lba_host::Window W = lba_host::build(M, 1, 0u, 8, inv);
        CHECK(W.flags == 0 && W.n_local == 1 && W.n_fixed == 2 && W.num_fixed == 2);
        CHECK(W.pose_kf == std::vector<int32_t>({2, 0, 1}) && W.hidx == std::vector<int32_t>({-1, -1, 0}) && W.pose_local == std::vector<int32_t>({0, 0, 1}));
        CHECK(W.point_mp == std::vector<int32_t>({0, 1}) && W.lm_start == std::vector<int32_t>({0, 2, 4}));
        CHECK(W.edges.size() == 4 && W.edges[0].pose == 2 && W.edges[1].pose == 1 && W.edges[2].pose == 1 && W.edges[3].pose == 0);
        CHECK(W.edges[2].kind == LBA_EDGE_STEREO && W.edges[2].obs[2] == 30.5f && W.edges[2].inv_sigma2 == inv[1] && W.edges[0].obs[0] == 100.f);
        CHECK(W.pose_start == std::vector<int32_t>({0, 1, 3, 4}) && W.pose_edges == std::vector<int32_t>({3, 1, 2, 0}));
        CHECK(W.poses[7] == 1.0 && W.poses[7 + 6] == 1.0 && W.poses[7 + 3] == 0.0);   // the identity: t = (1, 0, 0), q = (0, 0, 0, 1)
        // apply: the stereo edge of point 1 is an outlier: nObs 3 - 2 = 1 <= 2 -> bad; its record in key frame 2 dies by the point
        lba_host::Window O = W;
        O.poses[14] = 2.5;   // the one local pose moves: tcw = (2.5, 0, 0), Ow = (-2.5, 0, 0)
        const double chi2[4] = {1, 1, 9, 1}, depth[4] = {1, 1, 1, 1};
        const lba_host::Applied A = lba_host::apply(M, O, chi2, depth, sf, 8);
        CHECK(!A.early && A.erased.size() == 1 && A.erased[0] == std::make_pair(0, 1) && A.went_bad == std::vector<int>({1}));
        CHECK((M.mp[1].flags & ORBM_MP_BAD) && M.nobs[1] == 1 && M.kf_mp == std::vector<int32_t>({0, -1, 0, -1, -1}));
        CHECK(M.obs_start == std::vector<int32_t>({0, 2, 2}) && M.ref[1].ref_kf == 0);
        CHECK(M.pose[1].tcw[0] == 2.5f && M.center[1].left[0] == -2.5f && M.pose[0].tcw[0] == 1.f);
        // point 0 at (0, 0, 4): rays from (-2.5, 0, 0) and (-1, 0, 0); the reference key frame is slot 1, level 0
        const float d = (float)std::sqrt(2.5 * 2.5 + 16.0);
        CHECK(M.mp[0].max_distance == d && M.mp[0].min_distance == d / sf[7] && M.mp[0].normal[1] == 0.f && M.mp[0].normal[0] > 0.f);
        // half the edges outliers: the early return
        lba_host::Map M2 = M;
        const double chi2b[4] = {9, 9, 1, 1};
        const lba_host::Window W2 = lba_host::build(M2, 1, 0u, 8, inv);
        CHECK(W2.edges.size() == 2);
        const lba_host::Applied A2 = lba_host::apply(M2, W2, chi2b, depth, sf, 8);
        CHECK(A2.early && A2.erased.size() == 2 && M2.kf_mp == M.kf_mp);
    }
    {   // a synthetic world: the invariants of a window
        const lba_synth::World S = lba_synth::make(3, 6, 40, 150, 3, 20);
        const lba_host::Window W = lba_host::build(S.M, S.current, S.init_id, S.nlevels, S.inv_sigma2);
        CHECK(W.flags == 0 && W.n_local + W.n_fixed == (int)W.hidx.size() && W.lm_start.back() == (int)W.edges.size());
        for (size_t i = 1; i < W.pose_kf.size(); i++) CHECK(S.M.ckf[W.pose_kf[i - 1]].id < S.M.ckf[W.pose_kf[i]].id);
        for (size_t i = 0; i < W.hidx.size(); i++)
            for (int j = W.pose_start[i]; j < W.pose_start[i + 1]; j++) CHECK(W.edges[W.pose_edges[j]].pose == (int)i && (j == W.pose_start[i] || W.pose_edges[j - 1] < W.pose_edges[j]));
    }
    std::printf("local_ba_host_test OK\n");
    return 0;
}
