// new_keyframe_host_test.cpp — the host restatement (new_keyframe_host.h) alone, on a hand-made map with a worked-out answer and on random
// worlds whose invariants are checked; links no library, so it also runs under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstdio>
#include <cstdlib>

#include "new_keyframe_synth.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// a key frame whose features hold `points`; feature i of key frame k has the descriptor of `ones[i]` leading one bits
static void add_kf(newkf_host::Map& M, const std::vector<int>& points, const std::vector<int>& ones, bool stereo, float x) {
    orbm_localmap_keyframe k;
    std::memset(&k, 0, sizeof k);
    k.flags = ORBM_LM_KF_PRESENT; k.parent = k.prev = -1; k.mp_row0 = (int)M.kf_mp.size(); k.n_feat = (int)points.size();
    orbm_cull_keyframe c;
    std::memset(&c, 0, sizeof c);
    c.id = 100u + (uint32_t)M.kf.size(); c.prev = c.next = -1; c.desc_row0 = k.mp_row0;
    orbm_keyframe_center ce;
    std::memset(&ce, 0, sizeof ce);
    ce.left[0] = ce.right[0] = x;
    for (size_t i = 0; i < points.size(); i++) {
        M.kf_mp.push_back(points[i]);
        M.feat.push_back(stereo ? (uint8_t)ORBM_CULL_FEAT_STEREO : (uint8_t)0);
        std::vector<uint8_t> d(32, 0);
        for (int b = 0; b < ones[i]; b++) d[b >> 3] |= (uint8_t)(1u << (b & 7));
        M.kf_desc.insert(M.kf_desc.end(), d.begin(), d.end());
    }
    M.kf.push_back(k); M.ckf.push_back(c); M.center.push_back(ce);
}

static void add_mp(newkf_host::Map& M, int found, int visible, uint32_t first, uint32_t flags = 0) {
    orbm_map_point m;
    std::memset(&m, 0, sizeof m);
    m.pos[2] = 4.f; m.desc_row = (int)M.mp.size(); m.flags = ORBM_MP_VALID | ORBM_MP_HAS_OBS | flags;
    M.mp.push_back(m);
    M.mp_desc.insert(M.mp_desc.end(), 32, (uint8_t)0xEE);
    M.found.push_back(found); M.visible.push_back(visible); M.first.push_back(first);
    M.ref.push_back({0, 0});
}

int main() {
    float sf[8] = {1.f};
    for (int i = 1; i < 8; i++) sf[i] = sf[i - 1] * 1.2f;
    {   // Key frames 0 and 1 see the points 0, 1, 2 (descriptors of 10 / 20 and 12 / 20 and 40 / 41 ones); the new key frame 2 (stereo, at
        // x = 3) holds point 0 twice without a record, point 1 with its record, a null entry and the bad point 3.  Pointer order 1, 2, 0.
        newkf_host::Map M;
        add_kf(M, {0, 1, 2}, {10, 12, 40}, false, 0.f);
        add_kf(M, {0, 1, 2}, {20, 20, 41}, false, 0.f);
        add_kf(M, {0, 1, -1, 0, 3}, {21, 0, 0, 99, 0}, true, 3.f);
        add_mp(M, 1, 1, 100); add_mp(M, 1, 1, 100); add_mp(M, 1, 9, 102); add_mp(M, 1, 1, 100, ORBM_MP_BAD);
        M.kf_by_order = {1, 2, 0};
        // rows in rank order: key frame 1, (2,) 0
        M.obs = {{1, 3, 0u}, {0, 0, 0u}, {1, 4, 0u}, {2, 7, 0u}, {0, 1, 0u}, {1, 5, 0u}, {0, 2, 0u}};
        M.obs_start = {0, 2, 5, 7, 7};
        M.nobs = {2, 4, 2, 0};
        M.recent = {2};
        newkf_host::Result R;
        newkf_host::Mapper(M, sf, 8).process_new_keyframe(2, 8, 16, R);
        CHECK(R.flags == 0 && R.code == std::vector<uint8_t>({ORBM_NEWKF_CODE_ADDED, ORBM_NEWKF_CODE_PUSHED, ORBM_NEWKF_CODE_NONE,
                                                               ORBM_NEWKF_CODE_PUSHED_DUP, ORBM_NEWKF_CODE_BAD_POINT}));
        CHECK(R.sel == std::vector<int>({0}) && M.recent == std::vector<int>({2, 1, 0}) && R.pushed == 2 && R.n_obs == 8);
        CHECK(M.nobs == std::vector<int32_t>({4, 4, 2, 0}));                       // a stereo feature weighs 2
        CHECK(M.obs_start == std::vector<int32_t>({0, 3, 6, 8, 8}));
        CHECK(M.obs[0].kf == 1 && M.obs[1].kf == 2 && M.obs[1].desc_row == 6 && M.obs[2].kf == 0);   // at its rank: the middle
        // descriptors of 20, 21, 10 ones: the lower medians are 1, 1, 10 and the first of the two wins, key frame 1's
        CHECK(M.mp_desc[0] == 0xFF && M.mp_desc[1] == 0xFF && M.mp_desc[2] == 0x0F && M.mp_desc[3] == 0);
        // the normal: the mean of (0, 0, 1), (-3, 0, 4) / 5 and (0, 0, 1)
        CHECK(std::fabs(M.mp[0].normal[0] + 0.2f) < 1e-6f && std::fabs(M.mp[0].normal[2] - 2.8f / 3.f) < 1e-6f);
        CHECK(M.mp[0].max_distance == 4.f && M.mp[1].max_distance == 0.f);         // point 1 was not refreshed
        // MapPointCulling at key frame 2 (id 102): point 2 has found / visible = 1/9; point 1 is two key frames old with nObs 4 > 3; point 0 with
        // nObs 4 likewise; in monocular mode nThObs is 2
        newkf_host::Map M2 = M;
        newkf_host::Mapper(M, sf, 8).cull_map_points(2, false, 16, R);
        CHECK(R.code == std::vector<uint8_t>({ORBM_MPCULL_CODE_CULLED_RATIO, ORBM_MPCULL_CODE_KEPT, ORBM_MPCULL_CODE_KEPT}));
        CHECK(R.sel == std::vector<int>({2}) && M.recent == std::vector<int>({1, 0}) && (M.mp[2].flags & ORBM_MP_BAD));
        CHECK(M.kf_mp[2] == -1 && M.kf_mp[5] == -1 && M.obs_start == std::vector<int32_t>({0, 3, 6, 6, 6}) && M.nobs[2] == 2);
        M2.nobs[1] = 3; M2.found[2] = 9;
        newkf_host::Mapper(M2, sf, 8).cull_map_points(2, false, 16, R);
        CHECK(R.code == std::vector<uint8_t>({ORBM_MPCULL_CODE_KEPT, ORBM_MPCULL_CODE_CULLED_OBS, ORBM_MPCULL_CODE_KEPT}));
        CHECK(M2.kf_mp[1] == -1 && M2.kf_mp[4] == -1 && M2.kf_mp[7] == -1);
        // the CSR capacity: three records stay, a capacity of two does not hold, and then nothing changes
        newkf_host::Map M3 = M;
        M3.mp[1].flags &= ~ORBM_MP_BAD; M3.found[1] = 0; M3.recent = {1, 1};
        newkf_host::Mapper(M3, sf, 8).cull_map_points(2, false, 2, R);
        CHECK((R.flags & ORBM_NEWKF_OBS_OVERFLOW) && R.n_obs == 3 && M3.recent.size() == 2 && !(M3.mp[1].flags & ORBM_MP_BAD));
        newkf_host::Mapper(M3, sf, 8).cull_map_points(2, false, 3, R);
        CHECK(R.flags == 0 && R.code == std::vector<uint8_t>({ORBM_MPCULL_CODE_CULLED_RATIO, ORBM_MPCULL_CODE_ERASED_BAD}) && M3.recent.empty());
    }
    size_t added = 0, culled = 0;
    for (uint64_t seed = 1; seed <= 8; seed++) {   // invariants on random worlds
        newkf_synth::World W = newkf_synth::make(seed, 3 + (int)(seed % 6), 40, 60 + (int)seed * 7, 30);
        newkf_host::Map& M = W.M;
        const size_t obs0 = M.obs.size(), rec0 = M.recent.size();
        newkf_host::Result R;
        newkf_host::Mapper(M, W.sf, W.nlevels).process_new_keyframe(W.current, 1000, 100000, R);
        CHECK(R.flags == 0 && M.obs.size() == obs0 + R.sel.size() && (size_t)R.n_obs == M.obs.size() && M.recent.size() == rec0 + (size_t)R.pushed);
        added += R.sel.size();
        for (int p : R.sel) {   // the point has exactly one record of the key frame, at the first feature that holds it
            int n = 0;
            for (int o = M.obs_start[p]; o < M.obs_start[p + 1]; o++)
                if (M.obs[o].kf == W.current) { n++; CHECK(M.kf_mp[M.obs[o].desc_row] == p); }
            CHECK(n == 1);
        }
        newkf_host::Mapper(M, W.sf, W.nlevels).cull_map_points(W.current, seed & 1, 100000, R);
        culled += R.sel.size();
        for (int p : R.sel) CHECK((M.mp[p].flags & ORBM_MP_BAD) && M.obs_start[p] == M.obs_start[p + 1]);
        for (int p : M.recent) CHECK(!(M.mp[p].flags & ORBM_MP_BAD));
        for (size_t p = 0; p < M.mp.size(); p++)   // every record that is left is mirrored in its key frame's row
            for (int o = M.obs_start[p]; o < M.obs_start[p + 1]; o++) CHECK((M.mp[p].flags & ORBM_MP_BAD) || M.kf_mp[M.obs[o].desc_row] == (int)p);
    }
    CHECK(added > 50 && culled > 20);
    std::printf("new_keyframe_host_test OK (%zu added, %zu culled)\n", added, culled);
    return 0;
}
