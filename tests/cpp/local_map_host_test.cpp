// local_map_host_test.cpp — the host-only parts of the local-map tests: the host restatement of tests/cpp/local_map_host.h on hand-made maps
// with known answers (the parent branch's outer break, the stalled inertial chain, first occurrence wins, the in_view quirk) and on the
// synthetic map of local_map_synth.h.  Links no library, so that it also runs under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstdio>
#include <cstdlib>

#include "local_map_synth.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using namespace localmap_host;

struct Hand {
    localmap_synth::World W;
    void kf(std::vector<int> mp, std::vector<int> covis = {}, std::vector<int> children = {}, int parent = -1, bool bad = false, int prev = -1) {
        orbm_localmap_keyframe K;
        std::memset(&K, 0, sizeof K);
        K.flags = ORBM_LM_KF_PRESENT | (bad ? ORBM_LM_KF_BAD : 0u);
        K.parent = parent; K.prev = prev;
        K.mp_row0 = (int)W.kf_mp.size(); K.n_feat = (int)mp.size();
        W.kf_mp.insert(W.kf_mp.end(), mp.begin(), mp.end());
        for (int c = 0; c < 10; c++) K.covis[c] = c < (int)covis.size() ? covis[c] : -1;
        K.child_start = (int)W.children.size(); K.n_child = (int)children.size();
        W.children.insert(W.children.end(), children.begin(), children.end());
        W.kf.push_back(K);
    }
    // observations = the key frames that hold the point, in index order (= pointer order here)
    void finish(int n_mp, std::vector<int> bad_mp = {}) {
        W.mp.assign(n_mp, orbm_map_point{});
        W.track.assign(n_mp, orbm_track{});
        for (int p = 0; p < n_mp; p++) { W.mp[p].flags = ORBM_MP_VALID; W.track[p].in_view = 1; }
        for (int p : bad_mp) W.mp[p].flags |= ORBM_MP_BAD;
        W.obs_start.assign(n_mp + 1, 0);
        for (int p = 0; p < n_mp; p++) {
            for (int k = 0; k < (int)W.kf.size(); k++) {
                bool has = false;
                for (int i = 0; i < W.kf[k].n_feat; i++) has |= W.kf_mp[W.kf[k].mp_row0 + i] == p;
                if (has) W.obs.push_back(orbm_observation{k, 0, 0u});
            }
            W.obs_start[p + 1] = (int)W.obs.size();
        }
        W.order.resize(W.kf.size());
        for (size_t k = 0; k < W.kf.size(); k++) W.order[k] = (int)k;
    }
};

static Result run(const localmap_synth::World& W, std::vector<int32_t>& vote, int last_kf = -1, bool inertial = false,
                  std::vector<int32_t> dropped = {}) {
    Scratch S;
    Result R;
    const orbm_localmap_frame F{last_kf, inertial ? ORBM_LM_INERTIAL : 0u};
    update(W.map(), F, vote.data(), (int)vote.size(), vote.data(), (int)vote.size(), dropped.data(), (int)dropped.size(), W.track.data(), S, R);
    return R;
}

int main() {
    {   // the parent branch's break leaves the outer loop; a bad parent is still added; the first usable child is the third
        Hand H;
        H.kf({0}, {1, 0, 2}, {1, 0, 3}, 4); H.kf({}, {}, {}, -1, true); H.kf({}); H.kf({}); H.kf({}, {}, {}, -1, true); H.kf({0}, {6}); H.kf({});
        H.finish(2);
        std::vector<int32_t> vote{0};
        const Result R = run(H.W, vote);
        CHECK((R.local_kf == std::vector<int32_t>{0, 5, 2, 3, 4}) && R.ref_kf == 0 && R.max_votes == 1 && R.flags == 0);
    }
    {   // first occurrence wins in the reverse walk; bad points are nulled and never listed; only the dropped point loses in_view
        Hand H;
        H.kf({0, 1, 1, 2, -1, 6}); H.kf({2, 3, 0, 6, 4}); H.kf({9});
        H.finish(10, {6, 7});
        std::vector<int32_t> vote{0, 7, 3, -1, 8, 6};
        const Result R = run(H.W, vote, -1, false, {2, 5, -1});
        CHECK((vote == std::vector<int32_t>{0, -1, 3, -1, 8, -1}));
        CHECK((R.local_kf == std::vector<int32_t>{0, 1}) && (R.local_src == std::vector<int32_t>{2, 3, 0, 4, 1}));
        const bool seen[5] = {true, true, true, false, false};
        for (int j = 0; j < 5; j++) CHECK(((R.local_mp[j].flags & ORBM_MP_SEEN) != 0) == seen[j] && R.track[j].in_view == (j == 0 ? 0 : 1));
    }
    {   // the inertial chain stalls at a listed key frame
        Hand H;
        for (int k = 0; k < 10; k++) H.kf(k == 4 || k == 5 ? std::vector<int>{0} : std::vector<int>{}, {}, {}, -1, false, k - 1);
        H.finish(1);
        std::vector<int32_t> vote{0};
        CHECK((run(H.W, vote, 7, true).local_kf == std::vector<int32_t>{4, 5, 7, 6}));
        CHECK((run(H.W, vote, 3, true).local_kf == std::vector<int32_t>{4, 5, 3, 2, 1, 0}));
        CHECK((run(H.W, vote, 3, false).local_kf == std::vector<int32_t>{4, 5}));
        CHECK(run(H.W, vote, 30, true).flags == ORBM_LM_BAD_INDEX);
    }
    {   // the synthetic map: invariants of the result, the scratch marks reused over frames
        const localmap_synth::World W = localmap_synth::make(3, 60, 2000, 200);
        localmap_synth::Rng R(5);
        Scratch S;
        Result A, B;
        for (int f = 0; f < 4; f++) {
            std::vector<int32_t> vote = localmap_synth::frame_points(R, 2000, 300), again = vote;
            const orbm_localmap_frame F{R.below(60), f & 1 ? ORBM_LM_INERTIAL : 0u};
            update(W.map(), F, vote.data(), 300, vote.data(), 300, nullptr, 0, W.track.data(), S, A);
            Scratch fresh;
            update(W.map(), F, again.data(), 300, again.data(), 300, nullptr, 0, W.track.data(), fresh, B);
            CHECK(A.local_kf == B.local_kf && A.local_src == B.local_src && A.ref_kf == B.ref_kf && vote == again && A.flags == 0);
            CHECK(A.local_kf.size() > 10 && A.local_src.size() > 500 && A.local_mp.size() == A.local_src.size());
            std::vector<char> once(2000, 0);
            for (int p : A.local_src) { CHECK(!once[p] && !(W.mp[p].flags & ORBM_MP_BAD)); once[p] = 1; }
        }
    }
    std::printf("local_map_host_test OK\n");
    return 0;
}
