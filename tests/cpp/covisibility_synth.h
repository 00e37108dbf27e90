// covisibility_synth.h — small flattened maps for the covisibility tests (tests/cpp/covisibility_host_test.cpp, covisibility_test.cpp), built
// on the key-frame lists of keyframe_culling_synth.h, with the graph's key-frame records and a pointer order.
#ifndef COVISIBILITY_SYNTH_H
#define COVISIBILITY_SYNTH_H
#include <vector>

#include "covisibility_host.h"
#include "keyframe_culling_synth.h"

namespace covis_synth {

struct World {
    cull_synth::World base;
    std::vector<orbm_covis_keyframe> ckf;
    std::vector<int32_t> order;   // d_kf_by_order
    covis_host::Map map() const {
        covis_host::Map M;
        M.mp = base.mp.data(); M.n_mp = (int)base.mp.size(); M.obs_start = base.obs_start.data(); M.obs = base.obs.data();
        M.kf = base.kf.data(); M.n_kf = (int)base.kf.size(); M.kf_mp = base.kf_mp.data(); M.kf_by_order = order.data();
        return M;
    }
};

inline World make(const std::vector<std::vector<int>>& points, int n_mp, const std::vector<int>& order) {
    World W;
    W.base = cull_synth::make(points, n_mp);
    W.order.assign(order.begin(), order.end());
    W.ckf.resize(points.size());
    for (size_t k = 0; k < points.size(); k++) W.ckf[k] = orbm_covis_keyframe{(uint32_t)k, 0, ORBM_COVIS_KF_FIRST_CONNECTION, 0};
    return W;
}

// key frame 0 shares counts[j] points with key frame j + 1, each point with that one key frame only
inline World star(const std::vector<int>& counts, const std::vector<int>& order) {
    std::vector<std::vector<int>> points(counts.size() + 1);
    int p = 0;
    for (size_t j = 0; j < counts.size(); j++)
        for (int i = 0; i < counts[j]; i++, p++) { points[0].push_back(p); points[j + 1].push_back(p); }
    return make(points, p, order);
}

}  // namespace covis_synth
#endif
