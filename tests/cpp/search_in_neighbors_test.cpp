// search_in_neighbors_test.cpp — the header-only adapter orbslam3_hip::SearchInNeighbors (include/orbslam3_hip/LocalMapping.h) against the host
// restatement (tests/cpp/search_in_neighbors_host.h) on random worlds: targets, candidates, events, nFused, mpReplaced, the current key
// frame's points, the merged rows, and the slabs left on the device; the abort flag read through the pointer; capacities and refusals as
// exceptions.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "orbslam3_hip/LocalMapping.h"
#include "search_in_neighbors_synth.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using orbslam3_hip::SearchInNeighbors;

static SearchInNeighbors::MapView view_of(fusenb_host::Map& M, int max_feat) {
    SearchInNeighbors::MapView V;
    V.map.mapPoints = M.mp.data(); V.map.nMapPoints = (int)M.mp.size(); V.map.obsStart = M.obs_start.data(); V.map.observations = M.obs.data();
    V.map.nObservations = (int)M.obs.size(); V.map.keyFrames = M.kf.data(); V.map.nKeyFrames = (int)M.kf.size();
    V.map.keyFrameMapPoints = M.kf_mp.data(); V.map.nKeyFrameMapPointRows = (int)M.kf_mp.size(); V.map.cullKeyFrames = M.ckf.data();
    V.map.features = M.feat.data(); V.map.mapPointObservations = M.nobs.data();
    V.poses = M.pose.data(); V.keyPoints = M.kps.data(); V.uRight = M.u_right.data();
    V.keyFrameDescriptors = M.kf_desc.data(); V.nKeyFrameDescriptorRows = (int)(M.kf_desc.size() / 32);
    V.mapPointDescriptors = M.mp_desc.data(); V.nMapPointDescriptorRows = (int)(M.mp_desc.size() / 32);
    V.orderedKeyFrames = M.ordered_kf.data(); V.nOrdered = M.n_ordered.data(); V.capConnections = M.cap_conn;
    V.pointerOrder = M.kf_by_order.data(); V.fuseTargets = M.fuse_target.data(); V.found = M.found.data(); V.visible = M.visible.data();
    V.maxFeatures = max_feat;
    return V;
}

static SearchInNeighbors::Camera camera_of(const fusenb_synth::World& W) {
    SearchInNeighbors::Camera C;
    C.fx = W.P.fx; C.fy = W.P.fy; C.cx = W.P.cx; C.cy = W.P.cy; C.mbf = W.P.mbf; C.th = W.P.th;
    for (int i = 0; i < 4; i++) C.bounds[i] = W.P.bounds[i];
    C.grid = W.P.grid;
    C.scaleFactors.assign(W.P.scale_factors, W.P.scale_factors + W.P.nlevels);
    C.invLevelSigma2.assign(W.P.inv_level_sigma2, W.P.inv_level_sigma2 + W.P.nlevels);
    C.logScaleFactor = W.lsf;
    return C;
}

template <class T> static std::vector<T> fetch(const T* d, size_t n) {
    std::vector<T> h(n);
    if (n) orbslam3_hip::detail::download(h.data(), d, n * sizeof(T), nullptr);
    orbslam3_hip::detail::check(orb_stream_sync(nullptr), "sync");
    return h;
}

// one world through both; -> the number of events
static size_t compare(uint64_t seed, int n_kf, int n_true, bool mono, bool inertial, bool abort) {
    fusenb_synth::World W = fusenb_synth::make(seed, n_kf, n_true);
    fusenb_host::Map& M = W.M;
    SearchInNeighbors S;
    S.SetCamera(camera_of(W));
    S.SetMap(view_of(M, W.max_feat));
    SearchInNeighbors::Settings T;
    T.monocular = mono; T.inertial = inertial;
    T.capTargets = n_kf; T.capCandidates = (int)M.mp.size() + 1; T.capEvents = 2 * (int)M.kf_mp.size() + 1;
    T.capObservations = (int)(M.obs.size() + M.kf_mp.size());
    SearchInNeighbors::Result D;
    S.Run(W.current, T, &abort, D);

    orbm_fusenb_params P = W.P;
    P.current_kf = W.current;
    P.flags = (mono ? ORBM_FUSENB_MONOCULAR : 0u) | (inertial ? ORBM_FUSENB_INERTIAL : 0u) | (abort ? ORBM_FUSENB_ABORT_BA : 0u);
    fusenb_host::Result H;
    fusenb_host::Fuser(M, P, W.lsf, T.capTargets, T.capCandidates, T.capEvents).run(H);

    CHECK(D.flags == H.flags && D.targets == H.targets && D.targetsRequired == H.targets_required);
    CHECK(D.candidates == H.candidates && D.candidatesRequired == H.candidates_required && D.nFused == H.nfused);
    CHECK(D.events.size() == H.events.size());
    for (size_t i = 0; i < H.events.size(); i++) {
        const SearchInNeighbors::Event& e = D.events[i];
        CHECK((fusenb_host::Event{e.call, e.keyFrame, e.listIndex, e.point, e.feature, e.other, e.kind}) == H.events[i]);
    }
    CHECK(D.replaced == H.replaced && D.sel == H.sel && D.obsStart == H.obs_start && D.observations.size() == H.obs.size());
    CHECK(H.obs.empty() || std::memcmp(D.observations.data(), H.obs.data(), H.obs.size() * sizeof(orbm_observation)) == 0);
    // the device map after the fold
    const orbm_fusenb_out& O = S.deviceOutputs();
    CHECK(fetch(O.d_kf_mp, M.kf_mp.size()) == M.kf_mp && fetch(O.d_mp_nobs, M.nobs.size()) == M.nobs);
    CHECK(fetch(O.d_found, M.found.size()) == M.found && fetch(O.d_visible, M.visible.size()) == M.visible);
    CHECK(fetch(O.d_fuse_target, M.fuse_target.size()) == M.fuse_target);
    const std::vector<orbm_map_point> mp = fetch(O.d_mp, M.mp.size());
    const std::vector<uint8_t> desc = fetch(O.d_mp_desc, M.mp_desc.size());
    for (size_t p = 0; p < mp.size(); p++) {
        CHECK(mp[p].flags == M.mp[p].flags);
        if (!(mp[p].flags & ORBM_MP_BAD)) CHECK(std::memcmp(&desc[p * 32], &M.mp_desc[p * 32], 32) == 0);
    }
    return H.events.size();
}

template <class E, class F> static bool throws(F f) {
    try { f(); } catch (const E&) { return true; } catch (...) { return false; }
    return false;
}

int main() {
    size_t events = 0;
    for (uint64_t seed = 1; seed <= 6; seed++)
        events += compare(seed, 4 + (int)(seed * 3 % 9), 30 + (int)(seed * 17 % 60), seed & 1, seed % 3 == 0, seed == 4);
    CHECK(events > 100);
    {   // capacities and refusals
        fusenb_synth::World W = fusenb_synth::make(2, 6, 40);
        SearchInNeighbors S;
        SearchInNeighbors::Result D;
        SearchInNeighbors::Settings T;
        CHECK(throws<std::logic_error>([&] { S.Run(W.current, T, nullptr, D); }));   // no map
        S.SetCamera(camera_of(W));
        SearchInNeighbors::MapView V = view_of(W.M, W.max_feat);
        V.map.hasRig = true;
        CHECK(throws<std::invalid_argument>([&] { S.SetMap(V); }));
        V.map.hasRig = false; V.mixedSettings = true;
        CHECK(throws<std::invalid_argument>([&] { S.SetMap(V); }));
        V.mixedSettings = false;
        S.SetMap(V);
        S.Run(W.current, T, nullptr, D);   // the default capacities hold for a real map
        CHECK(D.flags == 0 && !D.events.empty());
        S.SetMap(V);
        T.capTargets = 1; T.capCandidates = 400; T.capEvents = 4000; T.capObservations = 4000;
        CHECK(throws<std::length_error>([&] { S.Run(W.current, T, nullptr, D); }));
        CHECK((D.flags & ORBM_FUSENB_TARGET_OVERFLOW) && D.events.empty() && D.targetsRequired > 1);
        CHECK(throws<std::runtime_error>([&] { S.Run(77, T, nullptr, D); }) && (D.flags & ORBM_FUSENB_BAD_INDEX));
    }
    std::printf("search_in_neighbors_test OK (%zu events)\n", events);
    return 0;
}
