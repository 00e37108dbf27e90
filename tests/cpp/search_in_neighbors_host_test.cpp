// search_in_neighbors_host_test.cpp — the host restatement (search_in_neighbors_host.h) alone, on a hand-made world with a worked-out answer
// and on random worlds whose invariants are checked; links no library, so it also runs under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstdio>
#include <cstdlib>

#include "search_in_neighbors_synth.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using fusenb_host::Event;

// Key frames at the origin looking along z; point p at (x, y, 5) projects to (160 + 40 x, 120 + 40 y), level 3 with max_distance = 1.5 |pos|.
static void add_kf(fusenb_host::Map& M, const std::vector<std::pair<float, int>>& feats /* (x, point) */) {
    orbm_localmap_keyframe k;
    std::memset(&k, 0, sizeof k);
    k.flags = ORBM_LM_KF_PRESENT; k.parent = -1; k.prev = -1; k.mp_row0 = (int)M.kf_mp.size(); k.n_feat = (int)feats.size();
    orbm_cull_keyframe c;
    std::memset(&c, 0, sizeof c);
    c.id = 100u + (uint32_t)M.kf.size(); c.prev = c.next = -1; c.desc_row0 = k.mp_row0;
    orbm_fusenb_pose p;
    std::memset(&p, 0, sizeof p);
    p.Rcw[0] = p.Rcw[4] = p.Rcw[8] = 1.f;
    for (const auto& f : feats) {
        orb_keypoint kp;
        std::memset(&kp, 0, sizeof kp);
        kp.x = 160.f + 40.f * f.first; kp.y = 120.f; kp.octave = 3;
        M.kps.push_back(kp); M.u_right.push_back(-1.f); M.feat.push_back(3); M.kf_mp.push_back(f.second);
        std::vector<uint8_t> d(32, (uint8_t)(17 * (int)f.first));
        M.kf_desc.insert(M.kf_desc.end(), d.begin(), d.end());
    }
    M.kf.push_back(k); M.ckf.push_back(c); M.pose.push_back(p);
}

static void add_mp(fusenb_host::Map& M, float x) {
    orbm_map_point m;
    std::memset(&m, 0, sizeof m);
    m.pos[0] = x; m.pos[2] = 5.f; m.normal[2] = 1.f;
    m.max_distance = 1.5f * std::sqrt(x * x + 25.f); m.min_distance = 0.1f; m.desc_row = (int)M.mp.size(); m.flags = ORBM_MP_VALID | ORBM_MP_HAS_OBS;
    M.mp.push_back(m);
    std::vector<uint8_t> d(32, (uint8_t)(17 * (int)x));
    M.mp_desc.insert(M.mp_desc.end(), d.begin(), d.end());
}

int main() {
    {   // current key frame 0 holds points 0 (x = 0) and 1 (x = 1); target 1 has the free feature at x = 0 and point 2 at x = 1, seen by
        // key frames 1, 2, 3: point 0 is added, point 1 (nObs 1) is replaced by point 2 (nObs 3); stage 2 finds every candidate in place.
        fusenb_host::Map M;
        add_kf(M, {{0.f, 0}, {1.f, 1}});
        add_kf(M, {{0.f, -1}, {1.f, 2}});
        add_kf(M, {{1.f, 2}});
        add_kf(M, {{1.f, 2}});
        add_mp(M, 0.f); add_mp(M, 1.f); add_mp(M, 1.f);
        M.obs = {{0, 0, 0u}, {0, 1, 0u}, {1, 3, 0u}, {2, 4, 0u}, {3, 5, 0u}};
        M.obs_start = {0, 1, 2, 5};
        M.nobs = {1, 1, 3}; M.found = {1, 2, 3}; M.visible = {4, 5, 6};
        M.kf_by_order = {0, 1, 2, 3};
        M.cap_conn = 2;
        M.ordered_kf = {1, -1, -1, -1, -1, -1, -1, -1};
        M.n_ordered = {1, 0, 0, 0};
        M.fuse_target.assign(4, 0u);
        fusenb_synth::World W = fusenb_synth::make(1, 2, 1);   // (for the camera)
        orbm_fusenb_params P = W.P;
        P.current_kf = 0; P.flags = 0;
        fusenb_host::Result R;
        fusenb_host::Fuser(M, P, W.lsf, 4, 8, 8).run(R);
        CHECK(R.flags == 0 && R.targets == std::vector<int>({1}) && M.fuse_target[1] == 100u);
        CHECK(R.events.size() == 2 && R.events[0] == (Event{0, 1, 0, 0, 0, -1, ORBM_FUSENB_EV_ADD}));
        CHECK(R.events[1] == (Event{0, 1, 1, 1, 1, 2, ORBM_FUSENB_EV_LIST_POINT_REPLACED}));
        CHECK(R.nfused == std::vector<int>({2, 0, 0, 0, 0}) && R.candidates == std::vector<int>({0, 2}));
        CHECK(R.replaced == std::vector<int>({-1, 2, -1}) && R.sel == std::vector<int>({0, 2}));
        CHECK(M.kf_mp == std::vector<int32_t>({0, 2, 0, 2, 2, 2}) && M.nobs == std::vector<int32_t>({2, 1, 4}));
        CHECK(M.found == std::vector<int32_t>({1, 2, 5}) && M.visible == std::vector<int32_t>({4, 5, 11}));
        CHECK(R.obs_start == std::vector<int32_t>({0, 2, 2, 6}) && (M.mp[1].flags & ORBM_MP_BAD) && !(M.mp[2].flags & ORBM_MP_BAD));
    }
    size_t events = 0;
    for (uint64_t seed = 1; seed <= 8; seed++) {   // invariants on random worlds
        fusenb_synth::World W = fusenb_synth::make(seed, 5 + (int)(seed % 7), 60);
        orbm_fusenb_params P = W.P;
        P.current_kf = W.current;
        P.flags = (seed & 1) ? ORBM_FUSENB_MONOCULAR : 0u;
        fusenb_host::Result R;
        fusenb_host::Fuser(W.M, P, W.lsf, 16, 1000, 4000).run(R);
        events += R.events.size();
        CHECK(R.flags == 0 && R.obs_start.size() == W.M.mp.size() + 1 && (size_t)R.obs_start.back() == R.obs.size());
        for (size_t p = 0; p < W.M.mp.size(); p++) {
            if (R.replaced[p] >= 0) CHECK((W.M.mp[p].flags & ORBM_MP_BAD) && R.obs_start[p] == R.obs_start[p + 1]);
            for (int o = R.obs_start[p]; o < R.obs_start[p + 1]; o++)   // every record is mirrored in its key frame's row
                CHECK(W.M.kf_mp[R.obs[o].desc_row] == (int)p || (W.M.mp[p].flags & ORBM_MP_BAD));
        }
    }
    CHECK(events > 100);
    std::printf("search_in_neighbors_host_test OK (%zu events)\n", events);
    return 0;
}
