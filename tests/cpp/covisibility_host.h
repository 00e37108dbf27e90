// covisibility_host.h — host restatement of KeyFrame::UpdateConnections (KeyFrame.cc:427-550), AddConnection (:228-241), UpdateBestCovisibles
// (:243-265) and the connection part of SetBadFlag (:675-678, 696-697) with EraseConnection (:793-807) over the flattened map of
// include/orbhip.h "Covisibility graph".  The weight map of a key frame is a vector in insertion order (the store's row format); pointer
// order is the rank of the key frame in kf_by_order.  Serial and literal: every AddConnection that changes a map rebuilds at once.
#ifndef COVISIBILITY_HOST_H
#define COVISIBILITY_HOST_H
#include <algorithm>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "orbhip.h"

namespace covis_host {

struct Map {   // the arrays of orbm_localmap_view plus the graph's own key-frame records
    const orbm_map_point* mp; int n_mp;
    const int32_t* obs_start; const orbm_observation* obs;
    const orbm_localmap_keyframe* kf; int n_kf;
    const int32_t* kf_mp;
    const int32_t* kf_by_order;
};

struct Graph {
    std::vector<orbm_covis_keyframe> ckf;
    std::vector<std::vector<orbm_covis_entry>> conn;   // mConnectedKeyFrameWeights
    std::vector<std::vector<int>> okf, ow;             // mvpOrderedConnectedKeyFrames, mvOrderedWeights
    std::vector<int> parent;
    std::vector<uint8_t> bad;                          // isBad()
    std::vector<int> rank;                             // of every key frame in pointer order
    explicit Graph(const Map& M, const std::vector<orbm_covis_keyframe>& c) : ckf(c), conn(M.n_kf), okf(M.n_kf), ow(M.n_kf), parent(M.n_kf, -1),
                                                                              bad(M.n_kf, 0), rank(M.n_kf, 0) {
        for (int k = 0; k < M.n_kf; k++) { bad[k] = (M.kf[k].flags & ORBM_LM_KF_BAD) ? 1 : 0; parent[k] = M.kf[k].parent; }
        for (int r = 0; r < M.n_kf; r++) rank[M.kf_by_order[r]] = r;
    }
    int find(int b, int key) const {
        for (size_t i = 0; i < conn[b].size(); i++)
            if (conn[b][i].kf == key) return (int)i;
        return -1;
    }
};

struct Update { int n_counter, nmax, kfmax; bool event; int parent; };

inline void update_best_covisibles(Graph& G, int b) {
    std::vector<std::pair<int, int>> vPairs;   // (weight, rank): pair<int, KeyFrame*> sorts by weight, then by pointer
    for (const orbm_covis_entry& e : G.conn[b]) vPairs.push_back(std::make_pair(e.weight, G.rank[e.kf]));
    std::sort(vPairs.begin(), vPairs.end());
    std::vector<int> byRank(G.rank.size());
    for (size_t k = 0; k < G.rank.size(); k++) byRank[G.rank[k]] = (int)k;
    G.okf[b].clear(); G.ow[b].clear();
    for (const auto& p : vPairs) {
        const int k = byRank[p.second];
        if (!G.bad[k]) { G.okf[b].insert(G.okf[b].begin(), k); G.ow[b].insert(G.ow[b].begin(), p.first); }   // push_front
    }
}

inline void add_connection(Graph& G, int b, int a, int weight) {
    const int at = G.find(b, a);
    if (at < 0) G.conn[b].push_back(orbm_covis_entry{a, weight});
    else if (G.conn[b][at].weight != weight) G.conn[b][at].weight = weight;
    else return;
    update_best_covisibles(G, b);
}

inline Update update_connections(const Map& M, Graph& G, int a, uint32_t init_kf_id) {
    std::map<int, int> KFcounter;   // keyed by pointer rank: its iteration order is the reference's
    const orbm_localmap_keyframe& A = M.kf[a];
    for (int i = 0; i < A.n_feat; i++) {
        const int p = M.kf_mp[A.mp_row0 + i];
        if (p < 0) continue;
        if (M.mp[p].flags & ORBM_MP_BAD) continue;
        for (int o = M.obs_start[p]; o < M.obs_start[p + 1]; o++) {
            const orbm_observation& r = M.obs[o];
            if ((r.flags & ORBM_OBS_RIGHT) && o > M.obs_start[p] && M.obs[o - 1].kf == r.kf) continue;   // the same mObservations entry
            if (G.ckf[r.kf].id == G.ckf[a].id || G.bad[r.kf] || G.ckf[r.kf].map_id != G.ckf[a].map_id) continue;
            KFcounter[G.rank[r.kf]]++;
        }
    }
    Update U{(int)KFcounter.size(), 0, -1, false, -1};
    if (KFcounter.empty()) return U;
    std::vector<std::pair<int, int>> vPairs;
    int rmax = -1;
    for (const auto& it : KFcounter) {
        const int k = M.kf_by_order[it.first];
        if (it.second > U.nmax) { U.nmax = it.second; U.kfmax = k; rmax = it.first; }
        if (it.second >= 15) { vPairs.push_back(std::make_pair(it.second, it.first)); add_connection(G, k, a, it.second); }
    }
    if (vPairs.empty()) { vPairs.push_back(std::make_pair(U.nmax, rmax)); add_connection(G, U.kfmax, a, U.nmax); }
    std::sort(vPairs.begin(), vPairs.end());
    G.conn[a].clear();
    for (const auto& it : KFcounter) G.conn[a].push_back(orbm_covis_entry{M.kf_by_order[it.first], it.second});
    G.okf[a].clear(); G.ow[a].clear();
    for (const auto& p : vPairs) { G.okf[a].insert(G.okf[a].begin(), M.kf_by_order[p.second]); G.ow[a].insert(G.ow[a].begin(), p.first); }
    if ((G.ckf[a].flags & ORBM_COVIS_KF_FIRST_CONNECTION) && G.ckf[a].id != init_kf_id) {
        G.parent[a] = G.okf[a].front();
        G.ckf[a].flags &= ~ORBM_COVIS_KF_FIRST_CONNECTION;
        U.event = true; U.parent = G.parent[a];
    }
    return U;
}

// KeyFrame::SetBadFlag's connection part for key frame k (not deferred)
inline void erase_connections(Graph& G, int k) {
    const std::vector<orbm_covis_entry> mine = G.conn[k];
    for (const orbm_covis_entry& e : mine) {
        const int at = G.find(e.kf, k);
        if (at < 0) continue;
        G.conn[e.kf].erase(G.conn[e.kf].begin() + at);
        update_best_covisibles(G, e.kf);
    }
    G.conn[k].clear();
    G.okf[k].clear(); G.ow[k].clear();
    G.bad[k] = 1;
}

}  // namespace covis_host
#endif
