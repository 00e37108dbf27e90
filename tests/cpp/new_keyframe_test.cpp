// new_keyframe_test.cpp — the header-only adapters orbslam3_hip::ProcessNewKeyFrame and orbslam3_hip::MapPointCulling
// (include/orbslam3_hip/LocalMapping.h) against the host restatement (tests/cpp/new_keyframe_host.h) on random worlds: the codes, the
// points that gained a record, the recent list, the culled points, and the slabs left on the device (the CSR, the map-point records, the
// descriptor rows, d_kf_mp, nObs); the hand-over of the device map from one adapter to the other; capacities and refusals as exceptions.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "new_keyframe_synth.h"
#include "orbslam3_hip/LocalMapping.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using orbslam3_hip::MapPointCulling;
using orbslam3_hip::NewKeyFrameMap;
using orbslam3_hip::NewKeyFrameSlabs;
using orbslam3_hip::ProcessNewKeyFrame;

static NewKeyFrameMap::MapView view_of(const newkf_host::Map& M, int max_feat) {
    NewKeyFrameMap::MapView V;
    V.map.mapPoints = M.mp.data(); V.map.nMapPoints = (int)M.mp.size(); V.map.obsStart = M.obs_start.data(); V.map.observations = M.obs.data();
    V.map.nObservations = (int)M.obs.size(); V.map.keyFrames = M.kf.data(); V.map.nKeyFrames = (int)M.kf.size();
    V.map.keyFrameMapPoints = M.kf_mp.data(); V.map.nKeyFrameMapPointRows = (int)M.kf_mp.size(); V.map.cullKeyFrames = M.ckf.data();
    V.map.features = M.feat.data(); V.map.mapPointObservations = M.nobs.data();
    V.refPoints = M.ref.data(); V.centers = M.center.data();
    V.keyFrameDescriptors = M.kf_desc.data(); V.nKeyFrameDescriptorRows = (int)(M.kf_desc.size() / 32);
    V.mapPointDescriptors = M.mp_desc.data(); V.nMapPointDescriptorRows = (int)(M.mp_desc.size() / 32);
    V.pointerOrder = M.kf_by_order.data(); V.found = M.found.data(); V.visible = M.visible.data(); V.firstKeyFrameIds = M.first.data();
    V.recent = M.recent; V.maxFeatures = max_feat;
    return V;
}

template <class T> static std::vector<T> fetch(const T* d, size_t n) {
    std::vector<T> h(n);
    if (n) orbslam3_hip::detail::download(h.data(), d, n * sizeof(T), nullptr);
    orbslam3_hip::detail::check(orb_stream_sync(nullptr), "sync");
    return h;
}

// the device map behind the slabs against the host's
static void compare_map(const NewKeyFrameSlabs& S, const newkf_host::Map& M) {
    CHECK(S.view.n_obs == (int)M.obs.size());
    CHECK(fetch(S.view.d_obs_start, M.obs_start.size()) == M.obs_start);
    const std::vector<orbm_observation> obs = fetch(S.view.d_obs, M.obs.size());
    CHECK(M.obs.empty() || std::memcmp(obs.data(), M.obs.data(), M.obs.size() * sizeof(orbm_observation)) == 0);
    CHECK(fetch(S.d_kf_mp, M.kf_mp.size()) == M.kf_mp && fetch(S.d_mp_nobs, M.nobs.size()) == M.nobs);
    const std::vector<orbm_map_point> mp = fetch(S.d_mp, M.mp.size());
    const std::vector<uint8_t> desc = fetch(S.d_mp_desc, M.mp_desc.size());
    for (size_t p = 0; p < mp.size(); p++) {
        CHECK(std::memcmp(&mp[p], &M.mp[p], sizeof(orbm_map_point)) == 0);
        CHECK(std::memcmp(&desc[p * 32], &M.mp_desc[p * 32], 32) == 0);
    }
    const int n = fetch(S.d_n_recent, 1)[0];
    CHECK(n == (int)M.recent.size());
    const std::vector<int32_t> lst = fetch(S.d_recent, (size_t)n);
    CHECK(std::vector<int>(lst.begin(), lst.end()) == M.recent);
}

// one world through both steps of both; -> added + culled
static size_t compare(uint64_t seed, int n_kf, int n_feat, int n_mp, bool mono) {
    newkf_synth::World W = newkf_synth::make(seed, n_kf, n_feat, n_mp, 40);
    newkf_host::Map& M = W.M;
    ProcessNewKeyFrame P;
    P.SetScaleFactors(std::vector<float>(W.sf, W.sf + W.nlevels));
    P.SetMap(view_of(M, W.max_feat));
    const int capRecent = P.deviceSlabs().capRecent, capObs = P.deviceSlabs().capObservations;
    ProcessNewKeyFrame::Result D;
    P.Run(W.current, D);
    newkf_host::Result H;
    newkf_host::Mapper(M, W.sf, W.nlevels).process_new_keyframe(W.current, capRecent, capObs, H);
    CHECK(D.flags == H.flags && D.added == H.sel && D.pushed == H.pushed && D.pushesRequired == H.push_required);
    CHECK(D.observationsRequired == H.n_obs && D.recentSize == (int)M.recent.size());
    CHECK(std::vector<uint8_t>(D.codes.begin(), D.codes.begin() + H.code.size()) == H.code);
    compare_map(P.deviceSlabs(), M);
    size_t n = H.sel.size();

    MapPointCulling C;
    C.UseDeviceMap(P.deviceSlabs());   // the map stays where it is
    MapPointCulling::Result E;
    C.Run(W.current, mono, E);
    newkf_host::Mapper(M, W.sf, W.nlevels).cull_map_points(W.current, mono, capObs, H);
    CHECK(E.flags == H.flags && E.codes == H.code && E.culled == H.sel && E.recent == M.recent && E.observationsRequired == H.n_obs);
    compare_map(C.deviceSlabs(), M);
    n += H.sel.size();

    P.UseDeviceMap(C.deviceSlabs());   // and back: the same key frame again finds every point in place
    P.Run(W.current, D);
    newkf_host::Mapper(M, W.sf, W.nlevels).process_new_keyframe(W.current, capRecent, capObs, H);
    CHECK(D.flags == H.flags && D.added.empty() && H.sel.empty() && D.pushed == H.pushed);
    compare_map(P.deviceSlabs(), M);
    return n;
}

template <class E, class F> static bool throws(F f) {
    try { f(); } catch (const E&) { return true; } catch (...) { return false; }
    return false;
}

int main() {
    size_t n = 0;
    for (uint64_t seed = 1; seed <= 6; seed++) n += compare(seed, 3 + (int)(seed * 3 % 9), 30 + (int)(seed * 37 % 300), 50 + (int)(seed * 91 % 400), seed & 1);
    CHECK(n > 100);
    {   // capacities and refusals
        newkf_synth::World W = newkf_synth::make(2, 5, 40, 80, 10);
        ProcessNewKeyFrame P;
        ProcessNewKeyFrame::Result D;
        CHECK(throws<std::logic_error>([&] { P.Run(W.current, D); }));   // no map
        CHECK(throws<std::invalid_argument>([&] { P.SetScaleFactors(std::vector<float>(17, 1.f)); }));
        P.SetScaleFactors(std::vector<float>(W.sf, W.sf + W.nlevels));
        NewKeyFrameMap::MapView V = view_of(W.M, W.max_feat);
        V.map.hasRig = true;
        CHECK(throws<std::invalid_argument>([&] { P.SetMap(V); }));
        V.map.hasRig = false;
        V.capObservations = (int)W.M.obs.size();   // no room for a new record
        P.SetMap(V);
        CHECK(throws<std::length_error>([&] { P.Run(W.current, D); }));
        CHECK((D.flags & ORBM_NEWKF_OBS_OVERFLOW) && D.added.empty() && D.observationsRequired > (int)W.M.obs.size());
        compare_map(P.deviceSlabs(), W.M);         // the map stays as given
        V.capObservations = 0; V.capRecent = (int)V.recent.size() + 1;
        P.SetMap(V);
        CHECK(throws<std::length_error>([&] { P.Run(W.current, D); }));
        CHECK((D.flags & ORBM_NEWKF_RECENT_OVERFLOW) && D.pushed == 1 && D.pushesRequired > 1 && D.recentSize == V.capRecent);
        CHECK(throws<std::runtime_error>([&] { P.Run(77, D); }) && (D.flags & ORBM_NEWKF_BAD_INDEX));
        MapPointCulling C;
        MapPointCulling::Result E;
        CHECK(throws<std::logic_error>([&] { C.Run(W.current, false, E); }));
        C.SetMap(view_of(W.M, W.max_feat));
        CHECK(throws<std::runtime_error>([&] { C.Run(-1, false, E); }) && (E.flags & ORBM_NEWKF_BAD_INDEX));
        // PushRecent: the entries that are not padding, behind the list
        C.SetMap(view_of(W.M, W.max_feat));
        const int32_t sel[5] = {7, 3, -1, 9, -1};
        orbslam3_hip::detail::DevBuf dsel;
        C.PushRecent(dsel.upload(sel, 5), 5);
        std::vector<int> want = W.M.recent;
        want.insert(want.end(), {7, 3, 9});
        const int cnt = fetch(C.deviceSlabs().d_n_recent, 1)[0];
        const std::vector<int32_t> lst = fetch(C.deviceSlabs().d_recent, (size_t)cnt);
        CHECK(std::vector<int>(lst.begin(), lst.end()) == want);
    }
    std::printf("new_keyframe_test OK (%zu points added or culled)\n", n);
    return 0;
}
