// new_keyframe_host.h — a host restatement of the association loop of LocalMapping::ProcessNewKeyFrame (LocalMapping.cc:375-411) with
// MapPoint::AddObservation (MapPoint.cc:160-195), UpdateNormalAndDepth (:485-558) and ComputeDistinctiveDescriptors (:372-460), and of
// LocalMapping::MapPointCulling (:435-494) with MapPoint::SetBadFlag (:254-277), over the flattened records of include/orbhip.h "New key
// frame".  Both loops are serial, as the reference's are; mObservations is a vector of (key frame, feature) kept in the rank order of
// d_kf_by_order.  Links no library: the adapter test compares the device against it, the timing tool times it, and
// new_keyframe_host_test.cpp runs it alone (also under ASan + UBSan).
#ifndef NEW_KEYFRAME_HOST_H
#define NEW_KEYFRAME_HOST_H
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "orbhip.h"

namespace newkf_host {

struct Map {
    // the view and the inputs, as the device gets them (a well-formed map: every record can be read)
    std::vector<orbm_map_point> mp;
    std::vector<int32_t> obs_start;
    std::vector<orbm_observation> obs;
    std::vector<orbm_localmap_keyframe> kf;
    std::vector<int32_t> kf_mp, kf_by_order;
    std::vector<orbm_cull_keyframe> ckf;
    std::vector<orbm_refresh_point> ref;
    std::vector<orbm_keyframe_center> center;
    std::vector<uint8_t> feat, kf_desc, mp_desc;
    std::vector<int32_t> nobs, found, visible;
    std::vector<uint32_t> first;
    std::vector<int> recent;   // mlpRecentAddedMapPoints
};

struct Result {
    std::vector<uint8_t> code;
    std::vector<int> sel;      // the points that gained a record / that were culled, in order
    int pushed = 0, push_required = 0, n_obs = 0;
    uint32_t flags = 0;
};

class Mapper {
public:
    Mapper(Map& m, const float* scale_factors, int nlevels) : M(m), sf(scale_factors), nl(nlevels) {
        const int n_kf = (int)M.kf.size(), n_mp = (int)M.mp.size();
        rank.assign(n_kf, 0);
        for (int r = 0; r < n_kf; r++) rank[M.kf_by_order[r]] = r;
        rows.resize(n_mp);
        for (int p = 0; p < n_mp; p++) {
            if (!(M.mp[p].flags & ORBM_MP_VALID)) continue;
            for (int o = M.obs_start[p]; o < M.obs_start[p + 1]; o++) rows[p].push_back({M.obs[o].kf, M.obs[o].desc_row - M.ckf[M.obs[o].kf].desc_row0});
            std::stable_sort(rows[p].begin(), rows[p].end(), [&](const Rec& a, const Rec& b) { return rank[a.first] < rank[b.first]; });
        }
    }

    // LocalMapping.cc:375-411.  cap_recent / cap_obs: the capacities the device call has
    void process_new_keyframe(int cur, int cap_recent, int cap_obs, Result& R) {
        R = Result();
        const orbm_localmap_keyframe& K = M.kf[cur];
        int n_obs = 0;
        for (const auto& r : rows) n_obs += (int)r.size();
        // (what the call would need is known before it writes: a first feature of a point without a record of the key frame adds one)
        std::vector<uint8_t> seen(M.mp.size(), 0);
        for (int i = 0; i < K.n_feat; i++) {
            const int p = M.kf_mp[K.mp_row0 + i];
            if (p >= 0 && !(M.mp[p].flags & ORBM_MP_BAD) && !in_kf(p, cur) && !seen[p]) { seen[p] = 1; n_obs++; }
        }
        R.n_obs = n_obs;
        const bool fits = n_obs <= cap_obs;
        if (!fits) R.flags |= ORBM_NEWKF_OBS_OVERFLOW;
        std::fill(seen.begin(), seen.end(), 0);
        std::vector<int> pushes;
        for (int i = 0; i < K.n_feat; i++) {
            const int p = M.kf_mp[K.mp_row0 + i];
            if (p < 0) { R.code.push_back(ORBM_NEWKF_CODE_NONE); continue; }
            if (M.mp[p].flags & ORBM_MP_BAD) { R.code.push_back(ORBM_NEWKF_CODE_BAD_POINT); continue; }
            if (!in_kf(p, cur) && !seen[p]) {
                seen[p] = 1;
                R.code.push_back(ORBM_NEWKF_CODE_ADDED);
                if (!fits) continue;
                add_observation(p, cur, i);
                update_normal_and_depth(p);
                compute_distinctive_descriptors(p, R);
                R.sel.push_back(p);
            } else {
                pushes.push_back(p);
                R.code.push_back(seen[p] ? ORBM_NEWKF_CODE_PUSHED_DUP : ORBM_NEWKF_CODE_PUSHED);
            }
        }
        R.push_required = (int)pushes.size();
        const int room = cap_recent - (int)M.recent.size();
        if (R.push_required > room) R.flags |= ORBM_NEWKF_RECENT_OVERFLOW;
        if (fits) {
            R.pushed = std::min(R.push_required, room);
            M.recent.insert(M.recent.end(), pushes.begin(), pushes.begin() + R.pushed);
            write_csr();
        }
    }

    // LocalMapping.cc:435-494
    void cull_map_points(int cur, bool monocular, int cap_obs, Result& R) {
        R = Result();
        const int th = monocular ? 2 : 3;
        const uint32_t cur_id = M.ckf[cur].id;
        // the chain, serially; SetBadFlag waits until the rows that stay are known to fit (they can only leave)
        std::vector<uint8_t> gone(M.mp.size(), 0);
        std::vector<int> kept;
        for (const auto& r : rows) R.n_obs += (int)r.size();
        for (int p : M.recent) {
            const int diff = (int)(cur_id - M.first[p]);
            if ((M.mp[p].flags & ORBM_MP_BAD) || gone[p]) R.code.push_back(ORBM_MPCULL_CODE_ERASED_BAD);
            else if ((float)M.found[p] / (float)M.visible[p] < 0.25f) { gone[p] = 1; R.sel.push_back(p); R.code.push_back(ORBM_MPCULL_CODE_CULLED_RATIO); }
            else if (diff >= 2 && M.nobs[p] <= th) { gone[p] = 1; R.sel.push_back(p); R.code.push_back(ORBM_MPCULL_CODE_CULLED_OBS); }
            else if (diff >= 3) R.code.push_back(ORBM_MPCULL_CODE_RETIRED);
            else { kept.push_back(p); R.code.push_back(ORBM_MPCULL_CODE_KEPT); }
        }
        R.push_required = (int)M.recent.size();
        for (int p : R.sel) R.n_obs -= (int)rows[p].size();
        if (R.n_obs > cap_obs) {
            R.flags |= ORBM_NEWKF_OBS_OVERFLOW;
            R.sel.clear();
            return;
        }
        for (int p : R.sel) set_bad_flag(p);
        M.recent = kept;
        R.pushed = (int)kept.size();
        write_csr();
    }

private:
    typedef std::pair<int, int> Rec;   // (key frame, leftIndex)
    Map& M;
    const float* sf;
    int nl;
    std::vector<int> rank;
    std::vector<std::vector<Rec>> rows;

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
    static float norm3(const float* d) {   // cv::norm: sqrt of the double dot product
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)d[k] * (double)d[k];
        return (float)std::sqrt(s);
    }
    int usable(int p) const {
        int n = 0;
        for (const Rec& r : rows[p]) n += !(M.kf[r.first].flags & ORBM_LM_KF_BAD);
        return n;
    }
    void add_observation(int p, int k, int idx) {
        auto it = rows[p].begin();
        while (it != rows[p].end() && rank[it->first] <= rank[k]) ++it;
        rows[p].insert(it, Rec(k, idx));
        M.nobs[p] += weight(k, idx);
        M.mp[p].flags = (M.mp[p].flags & ~ORBM_MP_HAS_OBS) | (M.nobs[p] > 0 ? ORBM_MP_HAS_OBS : 0u);
    }
    void update_normal_and_depth(int p) {
        if (usable(p) > ORBM_REFRESH_MAX_OBS) return;   // (orbm_refresh_map_points leaves such a point alone in both halves)
        orbm_map_point& m = M.mp[p];
        float normal[3] = {0, 0, 0};
        for (const Rec& r : rows[p]) {
            float d[3];
            for (int k = 0; k < 3; k++) d[k] = m.pos[k] - M.center[r.first].left[k];
            const float nr = norm3(d);
            for (int k = 0; k < 3; k++) normal[k] = normal[k] + d[k] / nr;
        }
        float PC[3];
        for (int k = 0; k < 3; k++) PC[k] = m.pos[k] - M.center[M.ref[p].ref_kf].left[k];
        const float dist = norm3(PC);
        m.max_distance = dist * sf[M.ref[p].level];
        m.min_distance = m.max_distance / sf[nl - 1];
        for (int k = 0; k < 3; k++) m.normal[k] = normal[k] / (float)rows[p].size();
    }
    void compute_distinctive_descriptors(int p, Result& R) {
        std::vector<const uint8_t*> d;
        for (const Rec& r : rows[p])
            if (!(M.kf[r.first].flags & ORBM_LM_KF_BAD)) d.push_back(kf_desc(r.first, r.second));
        const int N = (int)d.size();
        if (N == 0) return;
        if (N > ORBM_REFRESH_MAX_OBS) { R.flags |= ORBM_NEWKF_REFRESH_OVERFLOW; return; }
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
    void set_bad_flag(int p) {
        M.mp[p].flags |= ORBM_MP_BAD;
        for (const Rec& r : rows[p]) M.kf_mp[M.kf[r.first].mp_row0 + r.second] = -1;   // EraseMapPointMatch(leftIndex)
        rows[p].clear();
    }
    void write_csr() {
        M.obs.clear();
        for (size_t p = 0; p < rows.size(); p++) {
            M.obs_start[p] = (int32_t)M.obs.size();
            for (const Rec& r : rows[p])
                M.obs.push_back({r.first, M.ckf[r.first].desc_row0 + r.second, (M.kf[r.first].flags & ORBM_LM_KF_BAD) ? ORBM_OBS_KF_BAD : 0u});
        }
        M.obs_start[rows.size()] = (int32_t)M.obs.size();
    }
};

}  // namespace newkf_host
#endif
