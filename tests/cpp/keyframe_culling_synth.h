// keyframe_culling_synth.h — small flattened maps for the key-frame culling tests (tests/cpp/keyframe_culling_host_test.cpp,
// keyframe_culling_test.cpp): key frames given as lists of map-point indices, observations derived from them in key-frame order (the first
// feature that holds a point is the entry's leftIndex), one descriptor row per feature.
#ifndef KEYFRAME_CULLING_SYNTH_H
#define KEYFRAME_CULLING_SYNTH_H
#include <cstring>
#include <vector>

#include "keyframe_culling_host.h"

namespace cull_synth {

struct World {
    std::vector<orbm_map_point> mp;
    std::vector<int32_t> obs_start, kf_mp;
    std::vector<orbm_observation> obs;
    std::vector<orbm_localmap_keyframe> kf;
    std::vector<orbm_cull_keyframe> ckf;
    std::vector<uint8_t> feat;
    cull_host::Map map() const {
        cull_host::Map M;
        M.mp = mp.data(); M.n_mp = (int)mp.size(); M.obs_start = obs_start.data(); M.obs = obs.data(); M.n_obs = (int)obs.size();
        M.kf = kf.data(); M.n_kf = (int)kf.size(); M.kf_mp = kf_mp.data(); M.n_kf_mp_rows = (int)kf_mp.size(); M.ckf = ckf.data();
        M.feat = feat.data();
        return M;
    }
};

// points[k] = the map-point index of every feature of key frame k (-1 = none); every feature has `octave`, CLOSE and no STEREO unless
// stereo[k][i]; the key frames form a chain dt seconds and `spread` metres apart, ids = indices
inline World make(const std::vector<std::vector<int>>& points, int n_mp, double dt = 1.0, float spread = 1.f, int octave = 0,
                  const std::vector<std::vector<int>>* stereo = nullptr) {
    World W;
    const int n_kf = (int)points.size();
    W.kf.resize(n_kf); W.ckf.resize(n_kf);
    std::vector<std::vector<orbm_observation>> seen(n_mp);
    for (int k = 0; k < n_kf; k++) {
        orbm_localmap_keyframe& K = W.kf[k];
        std::memset(&K, 0, sizeof K);
        K.flags = ORBM_LM_KF_PRESENT; K.parent = -1; K.prev = k - 1;
        for (int c = 0; c < 10; c++) K.covis[c] = -1;
        K.mp_row0 = (int)W.kf_mp.size(); K.n_feat = (int)points[k].size();
        orbm_cull_keyframe& C = W.ckf[k];
        std::memset(&C, 0, sizeof C);
        C.timestamp = 100.0 + dt * k; C.id = (uint32_t)k; C.prev = k - 1; C.next = k + 1 < n_kf ? k + 1 : -1; C.desc_row0 = K.mp_row0;
        C.imu_pos[0] = spread * (float)k;
        for (size_t i = 0; i < points[k].size(); i++) {
            const int p = points[k][i];
            const bool st = stereo && (*stereo)[k][i];
            W.kf_mp.push_back(p);
            W.feat.push_back((uint8_t)(octave | ORBM_CULL_FEAT_CLOSE | (st ? ORBM_CULL_FEAT_STEREO : 0u)));
            if (p < 0 || p >= n_mp) continue;
            bool have = false;
            for (const orbm_observation& o : seen[p]) have = have || o.kf == k;
            if (!have) seen[p].push_back(orbm_observation{k, K.mp_row0 + (int)i, 0u});
        }
    }
    W.mp.resize(n_mp);
    W.obs_start.assign(1, 0);
    for (int p = 0; p < n_mp; p++) {
        std::memset(&W.mp[p], 0, sizeof W.mp[p]);
        W.mp[p].flags = ORBM_MP_VALID | (seen[p].empty() ? 0u : ORBM_MP_HAS_OBS);
        W.obs.insert(W.obs.end(), seen[p].begin(), seen[p].end());
        W.obs_start.push_back((int32_t)W.obs.size());
    }
    return W;
}

// n_kf key frames that all hold the points 0 .. nf-1
inline World shared(int n_kf, int nf, double dt = 1.0, float spread = 1.f) {
    std::vector<int> all(nf);
    for (int i = 0; i < nf; i++) all[i] = i;
    return make(std::vector<std::vector<int>>(n_kf, all), nf, dt, spread);
}

inline orbm_cull_problem problem(int current, int n_cand, int n_in_map, uint32_t flags, uint32_t init_id = 0xFFFFFFF0u) {
    orbm_cull_problem P;
    P.current_kf = current; P.init_kf_id = init_id; P.cand_start = 0; P.n_cand = n_cand; P.n_kf_in_map = n_in_map; P.flags = flags;
    return P;
}

}  // namespace cull_synth
#endif
