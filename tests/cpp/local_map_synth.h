// local_map_synth.h — a small synthetic map for the local-map C++ tests: key frames that see windows of the map, observations that agree with
// them in pointer order, a spanning tree, covisibility lists, a chain of mPrevKF.
#ifndef LOCAL_MAP_SYNTH_H
#define LOCAL_MAP_SYNTH_H
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "local_map_host.h"

namespace localmap_synth {

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 2654435761u + 88172645463325252ull) {}
    uint32_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
    bool chance(int percent) { return below(100) < percent; }
};

struct World {
    std::vector<orbm_map_point> mp;
    std::vector<int32_t> obs_start;
    std::vector<orbm_observation> obs;
    std::vector<orbm_localmap_keyframe> kf;
    std::vector<int32_t> kf_mp, children, order;
    std::vector<orbm_track> track;
    localmap_host::Map map() const {
        localmap_host::Map M;
        M.mp = mp.data(); M.n_mp = (int)mp.size(); M.obs_start = obs_start.data(); M.obs = obs.data(); M.n_obs = (int)obs.size();
        M.kf = kf.data(); M.n_kf = (int)kf.size(); M.kf_mp = kf_mp.data(); M.n_kf_mp_rows = (int)kf_mp.size();
        M.children = children.data(); M.n_children = (int)children.size(); M.kf_by_order = order.data();
        return M;
    }
};

inline World make(uint64_t seed, int n_kf, int n_mp, int n_feat) {
    Rng R(seed);
    World W;
    W.mp.resize(n_mp);
    W.track.resize(n_mp);
    for (int p = 0; p < n_mp; p++) {
        std::memset(&W.mp[p], 0, sizeof(orbm_map_point));
        std::memset(&W.track[p], 0, sizeof(orbm_track));
        W.mp[p].pos[0] = (float)p; W.mp[p].desc_row = p;
        W.mp[p].flags = ORBM_MP_VALID | ORBM_MP_HAS_OBS | (R.chance(4) ? ORBM_MP_BAD : 0u);
        W.track[p].proj_x = (float)R.below(700); W.track[p].in_view = R.below(2); W.track[p].level = R.below(8);
    }
    W.order.resize(n_kf);
    for (int k = 0; k < n_kf; k++) W.order[k] = k;
    for (int k = n_kf - 1; k > 0; k--) std::swap(W.order[k], W.order[R.below(k + 1)]);
    std::vector<int> rank(n_kf);
    for (int r = 0; r < n_kf; r++) rank[W.order[r]] = r;
    W.kf.resize(n_kf);
    std::vector<std::vector<int>> kids(n_kf), seen_in(n_mp);
    for (int k = 0; k < n_kf; k++) {
        orbm_localmap_keyframe& K = W.kf[k];
        std::memset(&K, 0, sizeof K);
        K.flags = ORBM_LM_KF_PRESENT | (R.chance(5) ? ORBM_LM_KF_BAD : 0u);
        K.parent = k ? R.below(k) : -1;
        K.prev = k - 1;
        if (k) kids[K.parent].push_back(k);
        K.mp_row0 = (int)W.kf_mp.size();
        K.n_feat = n_feat / 2 + R.below(n_feat / 2 + 1);
        const int span = std::min(2 * K.n_feat, n_mp), lo = R.below(std::max(n_mp - span, 1));
        std::vector<char> mine(n_mp, 0);
        for (int i = 0; i < K.n_feat; i++) {
            const int p = R.chance(30) ? -1 : lo + R.below(span);
            W.kf_mp.push_back(p);
            if (p >= 0 && !mine[p]) { mine[p] = 1; seen_in[p].push_back(k); }
        }
        const int nc = R.below(11);
        for (int c = 0; c < 10; c++) K.covis[c] = c < nc ? R.below(n_kf) : -1;
    }
    for (int k = 0; k < n_kf; k++) {
        std::sort(kids[k].begin(), kids[k].end(), [&](int a, int b) { return rank[a] < rank[b]; });
        W.kf[k].child_start = (int)W.children.size();
        W.kf[k].n_child = (int)kids[k].size();
        W.children.insert(W.children.end(), kids[k].begin(), kids[k].end());
    }
    W.obs_start.assign(n_mp + 1, 0);
    for (int p = 0; p < n_mp; p++) {
        std::sort(seen_in[p].begin(), seen_in[p].end(), [&](int a, int b) { return rank[a] < rank[b]; });
        for (int k : seen_in[p]) {
            W.obs.push_back(orbm_observation{k, 0, 0u});
            if (R.chance(20)) W.obs.push_back(orbm_observation{k, 0, ORBM_OBS_RIGHT});
        }
        W.obs_start[p + 1] = (int)W.obs.size();
    }
    return W;
}

inline std::vector<int32_t> frame_points(Rng& R, int n_mp, int n) {
    std::vector<int32_t> v(n);
    for (int i = 0; i < n; i++) v[i] = R.chance(30) ? -1 : R.below(n_mp);
    return v;
}

}  // namespace localmap_synth
#endif
