// keyframe_culling_test.cpp — the header-only adapter orbslam3_hip::KeyFrameCulling (include/orbslam3_hip/LocalMapping.h) against the host
// restatement (tests/cpp/keyframe_culling_host.h): exit codes, counts and the order of the cull events in both modes; the abort flag read
// through the pointer; the state left in the device workspace; UseDeviceMap; rigs and bad indices as exceptions.
#include <cstdio>
#include <cstdlib>

#include "keyframe_culling_synth.h"
#include "orbslam3_hip/LocalMapping.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using orbslam3_hip::KeyFrameCulling;

static KeyFrameCulling::MapView view_of(const cull_synth::World& W) {
    KeyFrameCulling::MapView MV;
    MV.mapPoints = W.mp.data(); MV.nMapPoints = (int)W.mp.size(); MV.obsStart = W.obs_start.data(); MV.observations = W.obs.data();
    MV.nObservations = (int)W.obs.size(); MV.keyFrames = W.kf.data(); MV.nKeyFrames = (int)W.kf.size(); MV.keyFrameMapPoints = W.kf_mp.data();
    MV.nKeyFrameMapPointRows = (int)W.kf_mp.size(); MV.cullKeyFrames = W.ckf.data(); MV.features = W.feat.data();
    return MV;
}

// Run() against cull_host::cull on the same inputs
static void compare(KeyFrameCulling& K, const cull_synth::World& W, int current, const std::vector<int>& cands, const KeyFrameCulling::Settings& S,
                    bool abort, KeyFrameCulling::Result& D, cull_host::Result& H) {
    const uint32_t fl = (S.inertial ? ORBM_CULL_INERTIAL : 0u) | (S.monocular ? ORBM_CULL_MONOCULAR : 0u) |
                        (S.imuInitialized ? ORBM_CULL_IMU_INITIALIZED : 0u) | (S.inertialBA2 ? ORBM_CULL_INERTIAL_BA2 : 0u) | (abort ? ORBM_CULL_ABORT_BA : 0u);
    const std::vector<int32_t> c32(cands.begin(), cands.end());
    cull_host::cull(W.map(), cull_synth::problem(current, (int)cands.size(), S.keyFramesInMap, fl, S.initKeyFrameId), c32.data(), (int)c32.size(), H);
    K.Run(current, cands, S, &abort, D);
    CHECK(D.flags == H.flags && D.codes == H.code);
    CHECK(D.nMPs == std::vector<int>(H.nmps.begin(), H.nmps.end()) && D.nRedundantObservations == std::vector<int>(H.nred.begin(), H.nred.end()));
    CHECK(D.events.size() == H.events.size());
    for (size_t i = 0; i < H.events.size(); i++)
        CHECK(D.events[i].keyFrame == H.events[i].kf && D.events[i].prev == H.events[i].prev && D.events[i].next == H.events[i].next);
}

int main() {
    KeyFrameCulling::Result D;
    cull_host::Result H;
    {   // not inertial: the chain of two, both orders, on one uploaded map; the final nObs and record states in the workspace
        const cull_synth::World W = cull_synth::shared(6, 40);
        KeyFrameCulling K;
        K.SetMap(view_of(W));
        KeyFrameCulling::Settings S;
        S.initKeyFrameId = 5; S.keyFramesInMap = 6;
        compare(K, W, 5, {0, 1, 2, 5}, S, false, D, H);
        CHECK(D.codes == std::vector<uint8_t>({ORBM_CULL_CODE_CULLED, ORBM_CULL_CODE_CULLED, ORBM_CULL_CODE_KEPT, ORBM_CULL_CODE_SKIPPED}));
        CHECK(D.events.size() == 2 && D.events[0].keyFrame == 0 && D.events[1].keyFrame == 1);
        orbm_cull_workspace_layout Y;
        CHECK(orbm_cull_workspace((int)W.kf.size(), (int)W.mp.size(), (int)W.obs.size(), &Y) == ORB_OK);
        std::vector<uint8_t> ws(Y.stride);
        orbslam3_hip::detail::download(ws.data(), K.deviceWorkspace(), Y.stride, nullptr);
        orbslam3_hip::detail::check(orb_stream_sync(nullptr), "sync");
        CHECK(std::memcmp(ws.data() + Y.nobs, H.nobs.data(), H.nobs.size() * 4) == 0);
        CHECK(std::memcmp(ws.data() + Y.kf_erased, H.kf_erased.data(), H.kf_erased.size()) == 0);
        const uint32_t* rec = (const uint32_t*)(ws.data() + Y.rec);
        for (size_t o = 0; o < H.rec.size(); o++) CHECK((rec[o] & 3u) == H.rec[o]);
        compare(K, W, 5, {2, 1, 0}, S, false, D, H);   // every problem starts from the map as given
        CHECK(D.events.size() == 2 && D.events[0].keyFrame == 2 && D.events[1].keyFrame == 1);
        compare(K, W, 5, {}, S, false, D, H);
        CHECK(D.codes.empty() && D.events.empty());
        // the same device map through UseDeviceMap
        KeyFrameCulling K2;
        K2.UseDeviceMap(K.deviceMap(), K.deviceInputs().d_ckf, K.deviceInputs().d_feat, nullptr);
        compare(K2, W, 5, {0, 1, 2}, S, false, D, H);
        CHECK(D.events.size() == 2);
    }
    {   // inertial: a relink changes the next candidate's t; the abort flag ends the loop after 21 candidates, read through the pointer
        const cull_synth::World W = cull_synth::shared(30, 70, 0.2);
        KeyFrameCulling K;
        K.SetMap(view_of(W));
        KeyFrameCulling::Settings S;
        S.inertial = true; S.monocular = true; S.initKeyFrameId = 0; S.keyFramesInMap = 30;
        compare(K, W, 29, {10, 11, 13, 0, 28}, S, false, D, H);
        CHECK(D.codes == std::vector<uint8_t>({ORBM_CULL_CODE_CULLED_IMU1, ORBM_CULL_CODE_KEPT_INERTIAL, ORBM_CULL_CODE_CULLED_IMU1,
                                               ORBM_CULL_CODE_SKIPPED, ORBM_CULL_CODE_KEPT_RECENT}));
        CHECK(D.events.size() == 2 && D.events[0].prev == 9 && D.events[0].next == 11 && D.events[1].prev == 12 && D.events[1].next == 14);
        std::vector<int> many;
        for (int i = 0; i < 24; i++) many.push_back(1 + (i % 3) * 4);   // 1, 5, 9 again and again: culled once, then skipped as bad
        compare(K, W, 29, many, S, true, D, H);
        CHECK(D.codes[2] == ORBM_CULL_CODE_CULLED_IMU1 && D.codes[20] == ORBM_CULL_CODE_SKIPPED && D.codes[23] == ORBM_CULL_CODE_SKIPPED);
        S.keyFramesInMap = 23;
        compare(K, W, 29, {3, 5, 7, 9}, S, false, D, H);
        CHECK(D.codes == std::vector<uint8_t>({ORBM_CULL_CODE_CULLED_IMU1, ORBM_CULL_CODE_CULLED_IMU1, ORBM_CULL_CODE_KEPT_FEW_KFS, ORBM_CULL_CODE_KEPT_FEW_KFS}));
    }
    {   // the break at the bottom: with the flag set, candidate #21 that is processed ends the loop; a null pointer reads as false
        const cull_synth::World W = cull_synth::shared(30, 5, 5.0);   // t = 10: every candidate stays (KEPT_INERTIAL)
        KeyFrameCulling K;
        K.SetMap(view_of(W));
        KeyFrameCulling::Settings S;
        S.inertial = true; S.monocular = true; S.initKeyFrameId = 0xFFFFFFF0u; S.keyFramesInMap = 30;
        const std::vector<int> cands(24, 3);
        compare(K, W, 29, cands, S, true, D, H);
        CHECK(D.codes[20] == ORBM_CULL_CODE_KEPT_INERTIAL && D.codes[21] == ORBM_CULL_CODE_NOT_VISITED);
        K.Run(29, cands, S, nullptr, D);
        CHECK(D.codes[23] == ORBM_CULL_CODE_KEPT_INERTIAL);
    }
    {   // exceptions: a rig, no map, an index out of range (the result is filled in before)
        cull_synth::World W = cull_synth::shared(6, 8);
        KeyFrameCulling K;
        KeyFrameCulling::Settings S;
        S.initKeyFrameId = 9; S.keyFramesInMap = 6;
        bool threw = false;
        try { K.Run(5, {0}, S, nullptr, D); } catch (const std::logic_error&) { threw = true; }
        CHECK(threw);
        KeyFrameCulling::MapView MV = view_of(W);
        MV.hasRig = true;
        threw = false;
        try { K.SetMap(MV); } catch (const std::invalid_argument&) { threw = true; }
        CHECK(threw);
        threw = false;
        try { KeyFrameCulling::FeatureByte(64, 1.f, 2.f, -1.f); } catch (const std::invalid_argument&) { threw = true; }
        CHECK(threw);
        CHECK(KeyFrameCulling::FeatureByte(3, 1.f, 2.f, -1.f) == (3 | ORBM_CULL_FEAT_CLOSE) && KeyFrameCulling::FeatureByte(0, 3.f, 2.f, 0.f) == ORBM_CULL_FEAT_STEREO);
        CHECK(KeyFrameCulling::FeatureByte(1, -1.f, 2.f, 5.f) == (1 | ORBM_CULL_FEAT_STEREO));
        W.kf_mp[2] = 1000;
        K.SetMap(view_of(W));
        threw = false;
        try { K.Run(5, {0, 77}, S, nullptr, D); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw && (D.flags & ORBM_CULL_BAD_INDEX) && D.codes.size() == 2 && D.codes[1] == ORBM_CULL_CODE_SKIPPED && D.nMPs[0] == 7);
        W.kf_mp[2] = 2;
        W.obs[3].flags = ORBM_OBS_RIGHT;
        K.SetMap(view_of(W));
        threw = false;
        try { K.Run(5, {0}, S, nullptr, D); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw && D.flags == ORBM_CULL_UNSUPPORTED);
    }
    std::printf("keyframe_culling_test OK\n");
    return 0;
}
