// new_keyframe_synth.h — random well-formed maps for the host restatement of new_keyframe_host.h: key frames with feature rows, points with
// records in pointer-rank order, the new key frame's row holding points with and without a record of it, twice in places, and a recent list
// whose points cover every exit of MapPointCulling.  Deterministic per seed (a 64-bit LCG: no <random> distribution, whose results vary).
#ifndef NEW_KEYFRAME_SYNTH_H
#define NEW_KEYFRAME_SYNTH_H
#include <cstdint>
#include <cstring>
#include <vector>

#include "new_keyframe_host.h"

namespace newkf_synth {

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
    float unit() { return (float)(next() & 0xFFFF) / 65536.0f; }
};

struct World {
    newkf_host::Map M;
    int current = 0, max_feat = 1, nlevels = 8;
    float sf[16];
};

// n_kf key frames of about n_feat features over n_mp points; the last key frame is the new one
inline World make(uint64_t seed, int n_kf, int n_feat, int n_mp, int n_recent) {
    World W;
    Rng R(seed);
    newkf_host::Map& M = W.M;
    W.sf[0] = 1.0f;
    for (int i = 1; i < 16; i++) W.sf[i] = W.sf[i - 1] * 1.2f;
    W.current = n_kf - 1;
    std::vector<std::vector<std::pair<int, int>>> recs(n_mp);   // per point (kf, idx), filled in key-frame order
    for (int k = 0; k < n_kf; k++) {
        orbm_localmap_keyframe kf;
        std::memset(&kf, 0, sizeof kf);
        const int nf = n_feat - R.below(n_feat / 8 + 1);
        kf.flags = ORBM_LM_KF_PRESENT | ((k != W.current && R.below(12) == 0) ? ORBM_LM_KF_BAD : 0u);
        kf.parent = kf.prev = -1; kf.mp_row0 = (int)M.kf_mp.size(); kf.n_feat = nf;
        orbm_cull_keyframe c;
        std::memset(&c, 0, sizeof c);
        c.id = 100u + (uint32_t)k; c.prev = c.next = -1; c.desc_row0 = kf.mp_row0;
        orbm_keyframe_center ce;
        for (int a = 0; a < 3; a++) { ce.left[a] = R.unit() - 0.5f; ce.right[a] = ce.left[a]; }
        std::vector<uint8_t> has(n_mp, 0);
        for (int i = 0; i < nf; i++) {
            int p = R.below(3) ? R.below(n_mp) : -1;
            M.feat.push_back((uint8_t)(R.below(8) | (R.below(3) == 0 ? ORBM_CULL_FEAT_STEREO : 0u)));
            for (int b = 0; b < 32; b++) M.kf_desc.push_back((uint8_t)R.next());
            // an old key frame holds a point once and has its record; the new one holds some twice, and has the record of one in three
            if (p >= 0 && k != W.current && has[p]) p = -1;
            if (p >= 0 && !has[p] && (k != W.current || R.below(3) == 0)) recs[p].push_back({k, i});
            if (p >= 0) has[p] = 1;
            M.kf_mp.push_back(p);
        }
        if (nf > W.max_feat) W.max_feat = nf;
        M.kf.push_back(kf); M.ckf.push_back(c); M.center.push_back(ce);
    }
    // the pointer order: a permutation that is not the identity
    for (int k = 0; k < n_kf; k++) M.kf_by_order.push_back(k);
    for (int k = n_kf - 1; k > 0; k--) std::swap(M.kf_by_order[k], M.kf_by_order[R.below(k + 1)]);
    std::vector<int> rank(n_kf);
    for (int r = 0; r < n_kf; r++) rank[M.kf_by_order[r]] = r;
    M.obs_start.push_back(0);
    for (int p = 0; p < n_mp; p++) {
        orbm_map_point m;
        std::memset(&m, 0, sizeof m);
        m.pos[0] = 4.f * R.unit() - 2.f; m.pos[1] = 2.f * R.unit() - 1.f; m.pos[2] = 4.f + 4.f * R.unit();
        m.normal[2] = 1.f; m.min_distance = 1.f; m.max_distance = 12.f; m.desc_row = p;
        m.flags = ORBM_MP_VALID | (R.below(10) == 0 ? ORBM_MP_BAD : 0u);
        std::stable_sort(recs[p].begin(), recs[p].end(), [&](const std::pair<int, int>& a, const std::pair<int, int>& b) { return rank[a.first] < rank[b.first]; });
        int nobs = 0;
        for (const auto& r : recs[p]) {
            const int row = M.kf[r.first].mp_row0 + r.second;
            M.obs.push_back({r.first, M.ckf[r.first].desc_row0 + r.second, (M.kf[r.first].flags & ORBM_LM_KF_BAD) ? ORBM_OBS_KF_BAD : 0u});
            nobs += (M.feat[row] & ORBM_CULL_FEAT_STEREO) ? 2 : 1;
        }
        if (nobs > 0) m.flags |= ORBM_MP_HAS_OBS;
        M.obs_start.push_back((int32_t)M.obs.size());
        M.mp.push_back(m);
        M.nobs.push_back(nobs);
        M.found.push_back(R.below(6)); M.visible.push_back(R.below(9));
        M.first.push_back(100u + (uint32_t)(n_kf - 1) - (uint32_t)R.below(5) + (R.below(9) == 0 ? 2u : 0u));
        orbm_refresh_point rp;
        rp.ref_kf = R.below(n_kf); rp.level = R.below(W.nlevels);
        M.ref.push_back(rp);
        for (int b = 0; b < 32; b++) M.mp_desc.push_back((uint8_t)R.next());
    }
    for (int i = 0; i < n_recent; i++) M.recent.push_back(R.below(n_mp));
    return W;
}

}  // namespace newkf_synth
#endif
