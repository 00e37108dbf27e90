// local_map_host.h — Tracking::UpdateLocalKeyFrames (Tracking.cc:3042-3244), Tracking::UpdateLocalPoints (:2998-3036) and the marking loop of
// Tracking::SearchLocalPoints (:2852-2872) restated on the host over the flattened map of include/orbhip.h "Local map": what a caller runs
// today before it uploads the local map points.  std::map keyed by pointer-order rank stands for map<KeyFrame*,int> keyframeCounter.
// Test and timing infrastructure; the product never includes it.
#ifndef LOCAL_MAP_HOST_H
#define LOCAL_MAP_HOST_H
#include <cstdint>
#include <map>
#include <vector>

#include "orbhip.h"

namespace localmap_host {

struct Map {
    const orbm_map_point* mp = nullptr; int n_mp = 0;
    const int32_t* obs_start = nullptr; const orbm_observation* obs = nullptr; int n_obs = 0;
    const orbm_localmap_keyframe* kf = nullptr; int n_kf = 0;
    const int32_t* kf_mp = nullptr; int n_kf_mp_rows = 0;
    const int32_t* children = nullptr; int n_children = 0;
    const int32_t* kf_by_order = nullptr;
};

struct Result {
    std::vector<int32_t> local_kf;          // mvpLocalKeyFrames
    int ref_kf = -1, max_votes = 0;         // pKFmax
    std::vector<int32_t> local_src;         // mvpLocalMapPoints
    std::vector<orbm_map_point> local_mp;   // their records, ORBM_MP_SEEN or-ed in
    std::vector<orbm_track> track;          // their track entries
    uint32_t flags = 0;                     // ORBM_LM_BAD_INDEX
};

struct Scratch {   // per-map marks, kept between frames like mnTrackReferenceForFrame / mnLastFrameSeen (a frame id instead of a clear)
    std::vector<int32_t> kf_listed, mp_listed, mp_seen, mp_dropped, rank_of;
    int32_t id = 0;
    void fit(const Map& M) {
        if ((int)kf_listed.size() != M.n_kf || (int)mp_listed.size() != M.n_mp) {
            kf_listed.assign(M.n_kf, 0); mp_listed.assign(M.n_mp, 0); mp_seen.assign(M.n_mp, 0); mp_dropped.assign(M.n_mp, 0);
            rank_of.assign(M.n_kf, -1);
            for (int r = 0; r < M.n_kf; r++)
                if (M.kf_by_order[r] >= 0 && M.kf_by_order[r] < M.n_kf) rank_of[M.kf_by_order[r]] = r;
            id = 0;
        }
    }
};

inline bool point_ok(const Map& M, int p) { return p >= 0 && p < M.n_mp && (M.mp[p].flags & ORBM_MP_VALID); }
inline bool kf_present(const Map& M, int v) { return v >= 0 && v < M.n_kf && (M.kf[v].flags & ORBM_LM_KF_PRESENT); }

// vote / frame: in/out (bad points are nulled); frame may be the very array vote.  slab: the persistent track entries, [n_mp].
inline void update(const Map& M, const orbm_localmap_frame& F, int32_t* vote, int n_vote, int32_t* frame, int n_frame, const int32_t* dropped,
                   int n_dropped, const orbm_track* slab, Scratch& S, Result& R) {
    S.fit(M);
    const int32_t id = ++S.id;
    R.local_kf.clear(); R.local_src.clear(); R.local_mp.clear(); R.track.clear();
    R.ref_kf = -1; R.max_votes = 0; R.flags = 0;
    // votes (:3050-3112)
    std::map<int, int> keyframeCounter;
    for (int i = 0; i < n_vote; i++) {
        const int p = vote[i];
        if (p == -1) continue;
        if (!point_ok(M, p)) { vote[i] = -1; R.flags |= ORBM_LM_BAD_INDEX; continue; }
        if (M.mp[p].flags & ORBM_MP_BAD) { vote[i] = -1; continue; }
        const int s = M.obs_start[p], e = M.obs_start[p + 1];
        if (s < 0 || e < s || e > M.n_obs) { R.flags |= ORBM_LM_BAD_INDEX; continue; }
        for (int o = s; o < e; o++) {
            const int k = M.obs[o].kf;
            if ((M.obs[o].flags & ORBM_OBS_RIGHT) && o > s && M.obs[o - 1].kf == k) continue;
            if (k < 0 || k >= M.n_kf || S.rank_of[k] < 0) { R.flags |= ORBM_LM_BAD_INDEX; continue; }
            keyframeCounter[S.rank_of[k]]++;
        }
    }
    // first level (:3131-3150)
    auto push = [&](int v) { R.local_kf.push_back(v); S.kf_listed[v] = id; };
    for (const auto& it : keyframeCounter) {
        const int k = M.kf_by_order[it.first];
        if (!kf_present(M, k)) { R.flags |= ORBM_LM_BAD_INDEX; continue; }
        if (M.kf[k].flags & ORBM_LM_KF_BAD) continue;
        if (it.second > R.max_votes) { R.max_votes = it.second; R.ref_kf = k; }
        push(k);
    }
    // second loop (:3155-3213)
    const size_t n1 = R.local_kf.size();
    for (size_t i = 0; i < n1; i++) {
        if (R.local_kf.size() > 80) break;
        const orbm_localmap_keyframe& K = M.kf[R.local_kf[i]];
        for (int c = 0; c < 10; c++) {
            const int v = K.covis[c];
            if (v == -1) continue;
            if (!kf_present(M, v)) { R.flags |= ORBM_LM_BAD_INDEX; continue; }
            if (!(M.kf[v].flags & ORBM_LM_KF_BAD) && S.kf_listed[v] != id) { push(v); break; }
        }
        if (K.n_child < 0 || K.child_start < 0 || K.n_child > M.n_children - K.child_start) R.flags |= ORBM_LM_BAD_INDEX;
        else
            for (int c = 0; c < K.n_child; c++) {
                const int v = M.children[K.child_start + c];
                if (!kf_present(M, v)) { R.flags |= ORBM_LM_BAD_INDEX; continue; }
                if (!(M.kf[v].flags & ORBM_LM_KF_BAD) && S.kf_listed[v] != id) { push(v); break; }
            }
        const int par = K.parent;
        if (par != -1) {
            if (!kf_present(M, par)) R.flags |= ORBM_LM_BAD_INDEX;
            else if (S.kf_listed[par] != id) { push(par); break; }
        }
    }
    // inertial tail (:3217-3236)
    if ((F.flags & ORBM_LM_INERTIAL) && R.local_kf.size() < 80) {
        int t = F.last_kf;
        for (int i = 0; i < 20; i++) {
            if (t == -1) break;
            if (!kf_present(M, t)) { R.flags |= ORBM_LM_BAD_INDEX; break; }
            if (S.kf_listed[t] != id) { push(t); t = M.kf[t].prev; }
        }
    }
    // the marking loop (:2852-2872) and the dropped points
    for (int i = 0; i < n_frame; i++) {
        const int p = frame[i];
        if (p == -1) continue;
        if (!point_ok(M, p)) { frame[i] = -1; R.flags |= ORBM_LM_BAD_INDEX; }
        else if (M.mp[p].flags & ORBM_MP_BAD) frame[i] = -1;
        else S.mp_seen[p] = id;
    }
    for (int i = 0; i < n_dropped; i++) {
        const int p = dropped[i];
        if (p == -1) continue;
        if (!point_ok(M, p)) R.flags |= ORBM_LM_BAD_INDEX;
        else S.mp_dropped[p] = id;
    }
    // UpdateLocalPoints (:2998-3036)
    for (size_t s = R.local_kf.size(); s-- > 0;) {
        const orbm_localmap_keyframe& K = M.kf[R.local_kf[s]];
        if (K.mp_row0 < 0 || K.n_feat < 0 || K.n_feat > M.n_kf_mp_rows - K.mp_row0) { R.flags |= ORBM_LM_BAD_INDEX; continue; }
        for (int i = 0; i < K.n_feat; i++) {
            const int p = M.kf_mp[K.mp_row0 + i];
            if (p == -1) continue;
            if (!point_ok(M, p)) { R.flags |= ORBM_LM_BAD_INDEX; continue; }
            if (S.mp_listed[p] == id) continue;
            if (M.mp[p].flags & ORBM_MP_BAD) continue;
            S.mp_listed[p] = id;
            R.local_src.push_back(p);
            orbm_map_point r = M.mp[p];
            orbm_track t = slab[p];
            if (S.mp_seen[p] == id || S.mp_dropped[p] == id) r.flags |= ORBM_MP_SEEN;
            if (S.mp_dropped[p] == id) t.in_view = 0;   // not for the frame's own points: the marking loop clears mbTrackInViewR (:2869)
            R.local_mp.push_back(r);
            R.track.push_back(t);
        }
    }
}

}  // namespace localmap_host
#endif
