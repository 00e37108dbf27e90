// search_in_neighbors_synth.h — random worlds for the SearchInNeighbors adapter test and the timing tool: key frames on a line looking at a
// cloud of true points, every true point held by one or two map points (so that fusions happen), the current key frame last.  Flattened
// as include/orbhip.h "Fusion in the neighbours" takes them.
#ifndef SEARCH_IN_NEIGHBORS_SYNTH_H
#define SEARCH_IN_NEIGHBORS_SYNTH_H
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "search_in_neighbors_host.h"

namespace fusenb_synth {

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint32_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
    double uni(double a = 0.0, double b = 1.0) { return a + (b - a) * (next() / 4294967296.0); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

struct World {
    fusenb_host::Map M;
    orbm_fusenb_params P;
    float lsf = 0;
    int current = 0, max_feat = 1;
};

// see: the chance that a key frame sees a true point in its image; max_feat: features per key frame at the most
inline World make(uint64_t seed, int n_kf, int n_true, double see = 0.75, int max_feat = 118) {
    World W;
    Rng rng(seed);
    fusenb_host::Map& M = W.M;
    orbm_fusenb_params& P = W.P;
    std::memset(&P, 0, sizeof P);
    P.fx = P.fy = 200.f; P.cx = 160.f; P.cy = 120.f; P.mbf = 20.f; P.th = 3.0f;
    P.bounds[0] = 0.f; P.bounds[1] = 320.f; P.bounds[2] = 0.f; P.bounds[3] = 240.f;
    P.grid = orbm_grid_params{0.f, 0.f, 64.f / 320.f, 48.f / 240.f};
    P.nlevels = 8;
    float sf[8] = {1.f};
    for (int i = 1; i < 8; i++) sf[i] = sf[i - 1] * 1.2f;
    for (int i = 0; i < 8; i++) { P.scale_factors[i] = sf[i]; P.inv_level_sigma2[i] = 1.0f / (sf[i] * sf[i]); }
    W.lsf = std::log(1.2f);
    W.current = n_kf - 1;

    struct True { double x, y, z; uint8_t d[32]; int oct; };
    std::vector<True> tp(n_true);
    for (True& t : tp) {
        t.x = rng.uni(-3, 4 + 0.25 * n_kf); t.y = rng.uni(-2, 2); t.z = rng.uni(4, 8); t.oct = 1 + rng.below(4);
        for (uint8_t& b : t.d) b = (uint8_t)rng.below(256);
    }
    M.kf.resize(n_kf); M.ckf.resize(n_kf); M.pose.resize(n_kf);
    std::vector<std::vector<std::pair<int, int>>> seen(n_true);   // (key frame, feature)
    std::vector<double> camx(n_kf);
    for (int k = 0; k < n_kf; k++) {
        camx[k] = 0.25 * k + rng.uni(-0.05, 0.05);
        std::memset(&M.kf[k], 0, sizeof M.kf[k]);
        std::memset(&M.ckf[k], 0, sizeof M.ckf[k]);
        std::memset(&M.pose[k], 0, sizeof M.pose[k]);
        M.kf[k].flags = ORBM_LM_KF_PRESENT; M.kf[k].parent = -1; M.kf[k].prev = k - 1;
        for (int& c : M.kf[k].covis) c = -1;
        M.kf[k].mp_row0 = (int)M.kf_mp.size();
        M.ckf[k].id = 100u + (uint32_t)k; M.ckf[k].prev = k - 1; M.ckf[k].next = k + 1 < n_kf ? k + 1 : -1; M.ckf[k].desc_row0 = M.kf[k].mp_row0;
        M.pose[k].Rcw[0] = M.pose[k].Rcw[4] = M.pose[k].Rcw[8] = 1.f;
        M.pose[k].Ow[0] = (float)camx[k]; M.pose[k].tcw[0] = -(float)camx[k];
        const bool stereo = rng.uni() < 0.5;
        int n = 0;
        for (int j = 0; j < n_true && n < max_feat - 1; j++) {
            const double u = 200 * (tp[j].x - camx[k]) / tp[j].z + 160, v = 200 * tp[j].y / tp[j].z + 120;
            if (!(u > 8 && u < 312 && v > 8 && v < 232) || rng.uni() > see) continue;
            for (int rep = rng.uni() < 0.12 ? 2 : 1; rep > 0; rep--, n++) {
                orb_keypoint kp;
                std::memset(&kp, 0, sizeof kp);
                kp.x = (float)(u + rng.uni(-0.4, 0.4)); kp.y = (float)(v + rng.uni(-0.4, 0.4)); kp.size = 31.f; kp.octave = tp[j].oct; kp.class_id = -1;
                M.kps.push_back(kp);
                const float ur = (stereo && rng.uni() < 0.8) ? (float)(u - 20.0 / tp[j].z) : -1.f;
                M.u_right.push_back(ur);
                M.feat.push_back((uint8_t)(tp[j].oct | (ur >= 0 ? ORBM_CULL_FEAT_STEREO : 0u)));
                uint8_t d[32];
                std::memcpy(d, tp[j].d, 32);
                for (int f = rng.below(9); f > 0; f--) { const int b = rng.below(256); d[b >> 3] ^= (uint8_t)(1 << (b & 7)); }
                M.kf_desc.insert(M.kf_desc.end(), d, d + 32);
                M.kf_mp.push_back(-1);
                seen[j].push_back({k, n});
            }
        }
        M.kf[k].n_feat = n;
        if (n > W.max_feat) W.max_feat = n;
    }
    // the map points: instances a / b of a true point among the other key frames, a / c / none in the current one
    std::vector<std::vector<std::pair<int, int>>> rows;
    for (int j = 0; j < n_true; j++) {
        int inst[3] = {-1, -1, -1};
        for (const auto& s : seen[j]) {
            const double r = rng.uni();
            int name;
            if (s.first == W.current) name = r < 0.4 ? 0 : (r < 0.7 ? 2 : -1);
            else name = r < 0.15 ? -1 : ((r < 0.6 || seen[j].size() < 3) ? 0 : 1);
            if (name < 0) continue;
            const int row = M.kf[s.first].mp_row0 + s.second;
            if (inst[name] < 0) {
                inst[name] = (int)M.mp.size();
                orbm_map_point mp;
                std::memset(&mp, 0, sizeof mp);
                const double dx = tp[j].x - camx[s.first], dist = std::sqrt(dx * dx + tp[j].y * tp[j].y + tp[j].z * tp[j].z);
                mp.pos[0] = (float)(tp[j].x + rng.uni(-0.004, 0.004)); mp.pos[1] = (float)(tp[j].y + rng.uni(-0.004, 0.004));
                mp.pos[2] = (float)(tp[j].z + rng.uni(-0.004, 0.004));
                mp.normal[0] = (float)(dx / dist); mp.normal[1] = (float)(tp[j].y / dist); mp.normal[2] = (float)(tp[j].z / dist);
                mp.max_distance = (float)(dist * sf[tp[j].oct]); mp.min_distance = mp.max_distance / sf[7];
                mp.desc_row = inst[name];
                mp.flags = ORBM_MP_VALID | (rng.uni() < 0.04 ? ORBM_MP_BAD : 0u);
                M.mp.push_back(mp);
                M.mp_desc.insert(M.mp_desc.end(), &M.kf_desc[(size_t)row * 32], &M.kf_desc[(size_t)row * 32] + 32);
                rows.emplace_back();
                M.found.push_back(1 + rng.below(8));
                M.visible.push_back(9 + rng.below(20));
            }
            M.kf_mp[row] = inst[name];
        }
    }
    // mObservations from the key frames' lists (the first feature that holds the point), in the rank order of a random pointer order
    M.kf_by_order.resize(n_kf);
    std::iota(M.kf_by_order.begin(), M.kf_by_order.end(), 0);
    for (int i = n_kf - 1; i > 0; i--) std::swap(M.kf_by_order[i], M.kf_by_order[rng.below(i + 1)]);
    M.nobs.assign(M.mp.size(), 0);
    for (int r = 0; r < n_kf; r++) {
        const int k = M.kf_by_order[r];
        for (int i = 0; i < M.kf[k].n_feat; i++) {
            const int p = M.kf_mp[M.kf[k].mp_row0 + i];
            if (p < 0 || (M.mp[p].flags & ORBM_MP_BAD) || (!rows[p].empty() && rows[p].back().first == k)) continue;
            rows[p].push_back({k, i});
            M.nobs[p] += (M.feat[M.kf[k].mp_row0 + i] & ORBM_CULL_FEAT_STEREO) ? 2 : 1;
        }
    }
    M.obs_start.assign(1, 0);
    for (size_t p = 0; p < M.mp.size(); p++) {
        for (const auto& r : rows[p]) M.obs.push_back(orbm_observation{r.first, M.ckf[r.first].desc_row0 + r.second, 0u});
        M.obs_start.push_back((int32_t)M.obs.size());
        if (M.nobs[p] > 0) M.mp[p].flags |= ORBM_MP_HAS_OBS;
    }
    // mvpOrderedConnectedKeyFrames by shared points
    std::vector<int> share((size_t)n_kf * n_kf, 0);
    for (const auto& rr : rows)
        for (const auto& a : rr)
            for (const auto& b : rr)
                if (a.first != b.first) share[(size_t)a.first * n_kf + b.first]++;
    M.cap_conn = n_kf > 1 ? n_kf - 1 : 1;
    M.ordered_kf.assign((size_t)n_kf * M.cap_conn, -1);
    M.n_ordered.assign(n_kf, 0);
    for (int k = 0; k < n_kf; k++) {
        std::vector<int> o;
        for (int b = 0; b < n_kf; b++) if (share[(size_t)k * n_kf + b] > 0) o.push_back(b);
        std::stable_sort(o.begin(), o.end(), [&](int a, int b) { return share[(size_t)k * n_kf + a] > share[(size_t)k * n_kf + b]; });
        for (size_t i = 0; i < o.size(); i++) M.ordered_kf[(size_t)k * M.cap_conn + i] = o[i];
        M.n_ordered[k] = (int)o.size();
    }
    M.fuse_target.assign(n_kf, 0u);
    return W;
}

}  // namespace fusenb_synth
#endif
