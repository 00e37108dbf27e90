// search_in_neighbors_host.h — a host restatement of LocalMapping::SearchInNeighbors (LocalMapping.cc:913-1043) with ORBmatcher::Fuse
// (ORBmatcher.cc:1630-1879), KeyFrame::GetFeaturesInArea (KeyFrame.cc:810-854), MapPoint::Replace (MapPoint.cc:286-338), AddObservation
// (:160-195) and ComputeDistinctiveDescriptors (:372-460) over the flattened records of include/orbhip.h "Fusion in the neighbours".
// mObservations is a vector of (key frame, feature) kept in the rank order of d_kf_by_order; Replace recomputes the survivor's descriptor inside
// itself, as the reference does.  Links no library: the adapter test compares the device against it, the timing tool times it, and
// search_in_neighbors_host_test.cpp runs it alone (also under ASan + UBSan).
#ifndef SEARCH_IN_NEIGHBORS_HOST_H
#define SEARCH_IN_NEIGHBORS_HOST_H
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "orbhip.h"

namespace fusenb_host {

struct Map {
    // the view and the inputs, as the device gets them
    std::vector<orbm_map_point> mp;
    std::vector<int32_t> obs_start;
    std::vector<orbm_observation> obs;
    std::vector<orbm_localmap_keyframe> kf;
    std::vector<int32_t> kf_mp, kf_by_order;
    std::vector<orbm_cull_keyframe> ckf;
    std::vector<orbm_fusenb_pose> pose;
    std::vector<uint8_t> feat, kf_desc, mp_desc;
    std::vector<orb_keypoint> kps;
    std::vector<float> u_right;
    std::vector<int32_t> ordered_kf, n_ordered, nobs, found, visible;
    std::vector<uint32_t> fuse_target;
    int cap_conn = 1;
};

struct Event { int call, kf, list_index, point, feature, other, kind; };
inline bool operator==(const Event& a, const Event& b) {
    return a.call == b.call && a.kf == b.kf && a.list_index == b.list_index && a.point == b.point && a.feature == b.feature && a.other == b.other &&
           a.kind == b.kind;
}

struct Result {
    std::vector<int> targets, candidates, nfused, replaced, sel;
    std::vector<Event> events;
    std::vector<int32_t> obs_start;
    std::vector<orbm_observation> obs;
    int targets_required = 0, candidates_required = 0;
    uint32_t flags = 0;
};

class Fuser {
public:
    Fuser(Map& m, const orbm_fusenb_params& p, float log_scale_factor, int cap_targets, int cap_candidates, int cap_events)
        : M(m), P(p), lsf(log_scale_factor), capT(cap_targets), capC(cap_candidates), capE(cap_events) {
        const int n_kf = (int)M.kf.size(), n_mp = (int)M.mp.size();
        rank.assign(n_kf, 0);
        for (int r = 0; r < n_kf; r++) rank[M.kf_by_order[r]] = r;
        rows.resize(n_mp);
        bad.resize(n_mp);
        for (int p = 0; p < n_mp; p++) {
            bad[p] = (M.mp[p].flags & ORBM_MP_BAD) != 0;
            for (int o = M.obs_start[p]; o < M.obs_start[p + 1]; o++)
                rows[p].push_back({M.obs[o].kf, M.obs[o].desc_row - M.ckf[M.obs[o].kf].desc_row0});
            std::stable_sort(rows[p].begin(), rows[p].end(), [&](const Rec& a, const Rec& b) { return rank[a.first] < rank[b.first]; });
        }
    }

    void run(Result& R) {
        const int cur = P.current_kf;
        const uint32_t cur_id = M.ckf[cur].id;
        const bool abort = P.flags & ORBM_FUSENB_ABORT_BA;
        std::vector<int> targets;
        auto usable = [&](int k) { return !((M.kf[k].flags & ORBM_LM_KF_BAD) || M.fuse_target[k] == cur_id); };
        auto take = [&](int k) { targets.push_back(k); M.fuse_target[k] = cur_id; };
        auto best = [&](int k, int n) { return std::min(n, M.n_ordered[k]); };
        for (int j = 0; j < best(cur, (P.flags & ORBM_FUSENB_MONOCULAR) ? 20 : 10); j++) {
            const int k = M.ordered_kf[(size_t)cur * M.cap_conn + j];
            if (usable(k)) take(k);
        }
        for (int i = 0, imax = (int)targets.size(); i < imax; i++) {
            for (int j = 0; j < best(targets[i], 20); j++) {
                const int k = M.ordered_kf[(size_t)targets[i] * M.cap_conn + j];
                if (usable(k) && M.ckf[k].id != cur_id) take(k);
            }
            if (abort) break;
        }
        if (P.flags & ORBM_FUSENB_INERTIAL)
            for (int k = M.kf[cur].prev; targets.size() < 20 && k != -1; k = M.kf[k].prev)
                if (usable(k)) take(k);
        R = Result();
        R.targets_required = (int)targets.size();
        R.nfused.assign(capT + 1, 0);
        R.replaced.assign(M.mp.size(), -1);
        res = &R;
        if ((int)targets.size() > capT) R.flags |= ORBM_FUSENB_TARGET_OVERFLOW;
        else {
            R.targets = targets;
            const int row0 = M.kf[cur].mp_row0, nf = M.kf[cur].n_feat;
            const std::vector<int> list(M.kf_mp.begin() + row0, M.kf_mp.begin() + row0 + nf);
            for (size_t t = 0; t < targets.size() && !stop; t++) R.nfused[t] = fuse(targets[t], list, (int)t);
            if (!abort && !stop) {
                std::vector<uint8_t> seen(M.mp.size(), 0);
                std::vector<int> cands;
                for (int k : targets)
                    for (int i = 0; i < M.kf[k].n_feat; i++) {
                        const int p = M.kf_mp[M.kf[k].mp_row0 + i];
                        if (p < 0 || bad[p] || seen[p]) continue;
                        seen[p] = 1;
                        cands.push_back(p);
                    }
                R.candidates_required = (int)cands.size();
                if ((int)cands.size() > capC) { R.flags |= ORBM_FUSENB_CANDIDATE_OVERFLOW; cands.resize(capC); }
                R.candidates = cands;
                R.nfused[targets.size()] = fuse(cur, cands, (int)targets.size());
            }
        }
        // the folded map
        for (int i = 0; i < M.kf[cur].n_feat; i++) {
            const int p = M.kf_mp[M.kf[cur].mp_row0 + i];
            if (p >= 0 && !bad[p] && std::find(R.sel.begin(), R.sel.end(), p) == R.sel.end()) R.sel.push_back(p);
        }
        R.obs_start.assign(1, 0);
        for (size_t p = 0; p < M.mp.size(); p++) {
            for (const Rec& r : rows[p])   // (ORBM_OBS_KF_BAD as the caller keeps it: the key frame's isBad(); a target never is)
                R.obs.push_back(orbm_observation{r.first, M.ckf[r.first].desc_row0 + r.second, (M.kf[r.first].flags & ORBM_LM_KF_BAD) ? ORBM_OBS_KF_BAD : 0u});
            R.obs_start.push_back((int32_t)R.obs.size());
            M.mp[p].flags = (M.mp[p].flags & ~ORBM_MP_HAS_OBS) | (M.nobs[p] > 0 ? ORBM_MP_HAS_OBS : 0u) | (bad[p] ? ORBM_MP_BAD : 0u);
        }
    }

private:
    typedef std::pair<int, int> Rec;   // (key frame, feature)
    Map& M;
    const orbm_fusenb_params P;
    const float lsf;
    const int capT, capC, capE;
    std::vector<int> rank;
    std::vector<std::vector<Rec>> rows;
    std::vector<uint8_t> bad;
    std::map<int, std::vector<std::vector<int>>> grids;
    Result* res = nullptr;
    bool stop = false;

    bool in_kf(int p, int k) const {
        for (const Rec& r : rows[p]) if (r.first == k) return true;
        return false;
    }
    int weight(int k, int idx) const { return (M.feat[M.kf[k].mp_row0 + idx] & ORBM_CULL_FEAT_STEREO) ? 2 : 1; }
    const uint8_t* kf_desc(int k, int idx) const { return &M.kf_desc[((size_t)M.ckf[k].desc_row0 + idx) * 32]; }
    static int hamming(const uint8_t* a, const uint8_t* b) {
        int s = 0;
        for (int i = 0; i < 32; i++) s += __builtin_popcount((unsigned)(a[i] ^ b[i]));
        return s;
    }
    void add_observation(int p, int k, int idx) {
        auto it = rows[p].begin();
        while (it != rows[p].end() && rank[it->first] <= rank[k]) ++it;
        rows[p].insert(it, Rec(k, idx));
        M.nobs[p] += weight(k, idx);
    }
    void compute_distinctive_descriptors(int p) {
        if (bad[p]) return;
        std::vector<const uint8_t*> d;
        for (const Rec& r : rows[p])
            if (!(M.kf[r.first].flags & ORBM_LM_KF_BAD)) d.push_back(kf_desc(r.first, r.second));
        const int N = (int)d.size();
        if (N == 0) return;
        if (N > ORBM_REFRESH_MAX_OBS) { res->flags |= ORBM_FUSENB_REFRESH_OVERFLOW; return; }
        int best_median = INT_MAX, best_idx = 0;
        std::vector<int> v(N);
        for (int i = 0; i < N; i++) {
            for (int j = 0; j < N; j++) v[j] = hamming(d[i], d[j]);
            std::sort(v.begin(), v.end());
            const int median = v[(int)(0.5 * (N - 1))];
            if (median < best_median) { best_median = median; best_idx = i; }
        }
        const int row = M.mp[p].desc_row;
        if (row >= 0 && (size_t)row * 32 < M.mp_desc.size()) std::memcpy(&M.mp_desc[(size_t)row * 32], d[best_idx], 32);
    }
    void replace(int a, int b) {
        if (a == b) return;
        const std::vector<Rec> obs = rows[a];
        rows[a].clear();
        bad[a] = 1;
        res->replaced[a] = b;
        for (const Rec& r : obs) {
            const int row = M.kf[r.first].mp_row0 + r.second;
            if (!in_kf(b, r.first)) { M.kf_mp[row] = b; add_observation(b, r.first, r.second); }
            else M.kf_mp[row] = -1;
        }
        if (!M.found.empty()) M.found[b] += M.found[a];
        if (!M.visible.empty()) M.visible[b] += M.visible[a];
        compute_distinctive_descriptors(b);
    }

    static float mat_row(const float* R, const float* X) {
        double s = 0.0;
        s += (double)R[0] * (double)X[0];
        s += (double)R[1] * (double)X[1];
        s += (double)R[2] * (double)X[2];
        return (float)s;
    }
    static double dot3(const float* a, const float* b) {
        double s = 0.0;
        s += (double)a[0] * (double)b[0];
        s += (double)a[1] * (double)b[1];
        s += (double)a[2] * (double)b[2];
        return s;
    }
    int predict_scale(float ratio) const {   // MapPoint::PredictScale with the host's logf; a non-finite ceil converts to INT_MIN on x86
        const float c = std::ceil(std::log(ratio) / lsf);
        const long long n = std::isfinite(c) ? (long long)c : (long long)INT_MIN;
        return n < 0 ? 0 : (n >= P.nlevels ? P.nlevels - 1 : (int)n);
    }
    const std::vector<std::vector<int>>& grid(int k) {   // AssignFeaturesToGrid with PosInGrid
        auto it = grids.find(k);
        if (it != grids.end()) return it->second;
        std::vector<std::vector<int>>& g = grids[k];
        g.resize(ORBM_GRID_COLS * ORBM_GRID_ROWS);
        for (int i = 0; i < M.kf[k].n_feat; i++) {
            const orb_keypoint& kp = M.kps[M.kf[k].mp_row0 + i];
            const int px = (int)std::round((kp.x - P.grid.min_x) * P.grid.grid_w_inv), py = (int)std::round((kp.y - P.grid.min_y) * P.grid.grid_h_inv);
            if (px < 0 || px >= ORBM_GRID_COLS || py < 0 || py >= ORBM_GRID_ROWS) continue;
            g[px * ORBM_GRID_ROWS + py].push_back(i);
        }
        return g;
    }

    int fuse(int k, const std::vector<int>& list, int call) {
        const orbm_fusenb_pose& F = M.pose[k];
        const int row0 = M.kf[k].mp_row0;
        const std::vector<std::vector<int>>& g = grid(k);
        int n_fused = 0;
        for (size_t i = 0; i < list.size(); i++) {
            const int p = list[i];
            if (p < 0 || bad[p] || in_kf(p, k)) continue;
            const orbm_map_point& mp = M.mp[p];
            const float xc = mat_row(F.Rcw, mp.pos) + F.tcw[0], yc = mat_row(F.Rcw + 3, mp.pos) + F.tcw[1], zc = mat_row(F.Rcw + 6, mp.pos) + F.tcw[2];
            if (zc < 0.0f) continue;
            const float invz = 1 / zc;
            const float u = P.fx * xc / zc + P.cx, v = P.fy * yc / zc + P.cy;
            if (!(u >= P.bounds[0] && u < P.bounds[1] && v >= P.bounds[2] && v < P.bounds[3])) continue;
            const float ur = u - P.mbf * invz;
            const float maxDistance = 1.2f * mp.max_distance, minDistance = 0.8f * mp.min_distance;
            const float PO[3] = {mp.pos[0] - F.Ow[0], mp.pos[1] - F.Ow[1], mp.pos[2] - F.Ow[2]};
            const float dist3D = (float)std::sqrt(dot3(PO, PO));
            if (dist3D < minDistance || dist3D > maxDistance) continue;
            if (dot3(PO, mp.normal) < 0.5 * dist3D) continue;
            const int level = predict_scale(mp.max_distance / dist3D);
            const float r = P.th * P.scale_factors[level];
            // KeyFrame::GetFeaturesInArea and the candidate loop
            const int x0 = std::max(0, (int)std::floor((u - P.grid.min_x - r) * P.grid.grid_w_inv));
            const int x1 = std::min(ORBM_GRID_COLS - 1, (int)std::ceil((u - P.grid.min_x + r) * P.grid.grid_w_inv));
            const int y0 = std::max(0, (int)std::floor((v - P.grid.min_y - r) * P.grid.grid_h_inv));
            const int y1 = std::min(ORBM_GRID_ROWS - 1, (int)std::ceil((v - P.grid.min_y + r) * P.grid.grid_h_inv));
            if (x0 >= ORBM_GRID_COLS || x1 < 0 || y0 >= ORBM_GRID_ROWS || y1 < 0) continue;
            const uint8_t* dMP = &M.mp_desc[(size_t)mp.desc_row * 32];
            int bestDist = 256, bestIdx = -1;
            for (int ix = x0; ix <= x1; ix++)
                for (int iy = y0; iy <= y1; iy++)
                    for (int idx : g[ix * ORBM_GRID_ROWS + iy]) {
                        const orb_keypoint& kp = M.kps[row0 + idx];
                        if (!(std::fabs(kp.x - u) < r && std::fabs(kp.y - v) < r)) continue;
                        const int kpLevel = kp.octave;
                        if (kpLevel < level - 1 || kpLevel > level) continue;
                        const float ex = u - kp.x, ey = v - kp.y;
                        if (M.u_right[row0 + idx] >= 0) {
                            const float er = ur - M.u_right[row0 + idx];
                            const float e2 = ex * ex + ey * ey + er * er;
                            if (e2 * P.inv_level_sigma2[kpLevel] > 7.8) continue;
                        } else {
                            const float e2 = ex * ex + ey * ey;
                            if (e2 * P.inv_level_sigma2[kpLevel] > 5.99) continue;
                        }
                        const int dist = hamming(dMP, kf_desc(k, idx));
                        if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
                    }
            if (bestDist > ORBM_TH_LOW) continue;
            if ((int)res->events.size() >= capE) { res->flags |= ORBM_FUSENB_EVENT_OVERFLOW; stop = true; break; }
            const int pin = M.kf_mp[row0 + bestIdx];
            int kind;
            if (pin >= 0) {
                if (bad[pin]) kind = ORBM_FUSENB_EV_NOOP_BAD;
                else if (pin == p) kind = ORBM_FUSENB_EV_NOOP_SAME;
                else if (M.nobs[pin] > M.nobs[p]) { kind = ORBM_FUSENB_EV_LIST_POINT_REPLACED; replace(p, pin); }
                else { kind = ORBM_FUSENB_EV_KF_POINT_REPLACED; replace(pin, p); }
            } else {
                kind = ORBM_FUSENB_EV_ADD;
                add_observation(p, k, bestIdx);
                M.kf_mp[row0 + bestIdx] = p;
            }
            res->events.push_back(Event{call, k, (int)i, p, bestIdx, pin, kind});
            n_fused++;
        }
        return n_fused;
    }
};

}  // namespace fusenb_host
#endif
