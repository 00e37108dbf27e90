// keyframe_culling_host_test.cpp — the host restatement of LocalMapping::KeyFrameCulling (tests/cpp/keyframe_culling_host.h) on hand-made maps
// whose answers are worked out in the comments.  Links no library; also built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>

#include "keyframe_culling_synth.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using cull_synth::problem;
typedef std::vector<uint8_t> Codes;
typedef std::vector<int32_t> Ints;

int main() {
    cull_host::Result R;
    {   // five key frames hold the same four points (nObs 5, four other observers): 0 is redundant and goes; 1 then has three others left
        const cull_synth::World W = cull_synth::shared(5, 4);
        const int32_t cands[2] = {0, 1};
        cull_host::cull(W.map(), problem(4, 2, 5, 0u), cands, 2, R);
        CHECK(R.flags == 0 && R.code == Codes({ORBM_CULL_CODE_CULLED, ORBM_CULL_CODE_KEPT}) && R.nmps == Ints({4, 4}) && R.nred == Ints({4, 0}));
        CHECK(R.events.size() == 1 && R.events[0].kf == 0 && R.events[0].prev == -1 && R.events[0].next == -1);
        CHECK(R.nobs == Ints({4, 4, 4, 4}) && R.kf_erased == Codes({1, 0, 0, 0, 0}) && R.kf_in_map == 4);
        for (int p = 0; p < 4; p++) CHECK(R.rec[5 * p] == ORBM_CULL_REC_ERASED_BY_KF && R.rec[5 * p + 1] == ORBM_CULL_REC_LIVE && !R.mp_bad[p]);
        const int32_t rev[2] = {1, 0};   // the other order culls the other one
        cull_host::cull(W.map(), problem(4, 2, 5, 0u), rev, 2, R);
        CHECK(R.kf_erased == Codes({0, 1, 0, 0, 0}) && R.events.size() == 1 && R.events[0].kf == 1);
    }
    {   // nMPs = 10, nRed = 9: 0.9f * 10 rounds to 9.0f, 9 > 9 is false: kept.  With ten redundant it goes.
        std::vector<int> ten(10), nine(9);
        for (int i = 0; i < 10; i++) { ten[i] = i; if (i < 9) nine[i] = i; }
        cull_synth::World W = cull_synth::make({ten, ten, nine, nine, nine, nine}, 10);
        const int32_t cands[1] = {0};
        cull_host::cull(W.map(), problem(5, 1, 6, 0u), cands, 1, R);
        CHECK(R.code == Codes({ORBM_CULL_CODE_KEPT}) && R.nmps == Ints({10}) && R.nred == Ints({9}) && R.events.empty());
        W = cull_synth::make({ten, ten, ten, ten, ten, ten}, 10);
        cull_host::cull(W.map(), problem(5, 1, 6, 0u), cands, 1, R);
        CHECK(R.code == Codes({ORBM_CULL_CODE_CULLED}));
    }
    {   // a point with three observers in the culled key frame goes bad: its other records die by the point; a stereo record weighs two
        const std::vector<int> good = {0, 1, 2, 3}, with = {0, 1, 2, 3, 4};
        cull_synth::World W = cull_synth::make({with, with, with, good, good, good}, 5);
        const int32_t cands[1] = {0};
        cull_host::cull(W.map(), problem(5, 1, 6, 0u), cands, 1, R);   // 4 redundant of 5: 4 > 4.5f is false
        CHECK(R.code == Codes({ORBM_CULL_CODE_KEPT}) && R.nmps == Ints({5}) && R.nred == Ints({4}));
        cull_host::cull(W.map(), problem(5, 1, 6, ORBM_CULL_INERTIAL), cands, 1, R);   // 0.5f: redundant; six key frames <= 21: kept
        CHECK(R.code == Codes({ORBM_CULL_CODE_KEPT_FEW_KFS}));
        W.ckf[0].prev = W.ckf[0].next = -1;
        cull_host::cull(W.map(), problem(5, 1, 30, ORBM_CULL_INERTIAL), cands, 1, R);
        CHECK(R.code == Codes({ORBM_CULL_CODE_KEPT_NO_NEIGHBOUR}));
        const std::vector<int> most = {0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 4};   // duplicates count per feature: 10 redundant of 11 > 9.9f
        W = cull_synth::make({most, with, with, good, good, good}, 5);
        cull_host::cull(W.map(), problem(5, 1, 6, 0u), cands, 1, R);
        CHECK(R.code == Codes({ORBM_CULL_CODE_CULLED}) && R.nmps == Ints({11}) && R.nred == Ints({10}));
        CHECK(R.nobs == Ints({5, 5, 5, 5, 2}) && R.mp_bad == Codes({0, 0, 0, 0, 1}));   // each observation erased once; point 4: 3 -> 2, bad
        const int s4 = W.obs_start[4];
        CHECK(R.rec[s4] == ORBM_CULL_REC_ERASED_BY_KF && R.rec[s4 + 1] == ORBM_CULL_REC_ERASED_BY_POINT && R.rec[s4 + 2] == ORBM_CULL_REC_ERASED_BY_POINT);
        const std::vector<std::vector<int>> st = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, {0, 0, 0, 0, 1}, {0, 0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        W = cull_synth::make({most, with, with, good, good, good}, 5, 1.0, 1.f, 0, &st);
        cull_host::cull(W.map(), problem(5, 1, 6, 0u), cands, 1, R);   // point 4: nObs 2 + 2 + 1 = 5 > 3 but only two others: not redundant
        CHECK(R.nred == Ints({10}) && R.nobs[4] == 3 && !R.mp_bad[4]);   // 5 - 2
    }
    {   // the inertial chain, 0.2 s apart: 3 goes (t = 0.4) and 22 -> 21 key frames make 5 a `continue`; 4's prev is 2 afterwards
        const cull_synth::World W = cull_synth::shared(30, 5, 0.2);
        const int32_t cands[2] = {3, 5};
        cull_host::cull(W.map(), problem(29, 2, 22, ORBM_CULL_INERTIAL | ORBM_CULL_MONOCULAR), cands, 2, R);
        CHECK(R.code == Codes({ORBM_CULL_CODE_CULLED_IMU1, ORBM_CULL_CODE_KEPT_FEW_KFS}) && R.kf_in_map == 21);
        CHECK(R.events.size() == 1 && R.events[0].kf == 3 && R.events[0].prev == 2 && R.events[0].next == 4);
        CHECK(R.prev[4] == 2 && R.next[2] == 4 && R.prev[3] == -1 && R.next[3] == -1);
        // 1 s apart: t = 2; only IMU_INITIALIZED and an id below last_ID (29 - 21 = 8) culls; 28 > 29 - 2 is recent
        const cull_synth::World V = cull_synth::shared(30, 5, 1.0);
        const int32_t c4[4] = {7, 8, 28, 0};
        cull_host::cull(V.map(), problem(29, 4, 30, ORBM_CULL_INERTIAL | ORBM_CULL_MONOCULAR | ORBM_CULL_IMU_INITIALIZED), c4, 4, R);
        CHECK(R.code == Codes({ORBM_CULL_CODE_CULLED_IMU1, ORBM_CULL_CODE_KEPT_INERTIAL, ORBM_CULL_CODE_KEPT_RECENT, ORBM_CULL_CODE_KEPT_NO_NEIGHBOUR}));
        // 0.02f metres apart: the norm as a double is below 0.02: the second branch; INERTIAL_BA2 switches it off
        const cull_synth::World U = cull_synth::shared(30, 5, 1.0, 0.02f);
        const int32_t c1[1] = {1};
        cull_host::cull(U.map(), problem(29, 1, 30, ORBM_CULL_INERTIAL | ORBM_CULL_MONOCULAR), c1, 1, R);
        CHECK(R.code == Codes({ORBM_CULL_CODE_CULLED_IMU2}));
        cull_host::cull(U.map(), problem(29, 1, 30, ORBM_CULL_INERTIAL | ORBM_CULL_MONOCULAR | ORBM_CULL_INERTIAL_BA2), c1, 1, R);
        CHECK(R.code == Codes({ORBM_CULL_CODE_KEPT_INERTIAL}));
    }
    {   // NOT_ERASE: deferred, nothing changes; a record of a key frame that is not there: flagged and absent; an empty candidate range
        cull_synth::World W = cull_synth::shared(5, 4);
        W.ckf[0].flags = ORBM_CULL_KF_NOT_ERASE;
        const int32_t cands[2] = {0, 1};
        cull_host::cull(W.map(), problem(4, 2, 5, 0u), cands, 2, R);
        CHECK(R.code == Codes({ORBM_CULL_CODE_CULLED | ORBM_CULL_CODE_DEFERRED, ORBM_CULL_CODE_CULLED}) && R.events.size() == 2);
        CHECK(R.kf_erased == Codes({0, 1, 0, 0, 0}) && R.nobs == Ints({4, 4, 4, 4}));
        W.obs[2].kf = 99;
        cull_host::cull(W.map(), problem(4, 2, 5, 0u), cands, 2, R);
        CHECK(R.flags == ORBM_CULL_BAD_INDEX && R.rec[2] == ORBM_CULL_REC_ABSENT && R.nred == Ints({3, 3}));   // point 0 has three others
        cull_host::cull(W.map(), problem(9, 2, 5, 0u), cands, 2, R);
        CHECK((R.flags & ORBM_CULL_BAD_INDEX) && R.code == Codes({0, 0}) && R.events.empty());
        cull_host::cull(W.map(), problem(4, 3, 5, 0u), cands, 2, R);
        CHECK((R.flags & ORBM_CULL_BAD_INDEX) && R.code.empty());
    }
    std::printf("keyframe_culling_host_test OK\n");
    return 0;
}
