// local_map_test.cpp — the header-only adapter orbslam3_hip::LocalMap (include/orbslam3_hip/Tracking.h) against the host restatement of the
// three reference functions (tests/cpp/local_map_host.h): key-frame list, pKFmax, point indices, the nulled lists, and the records and track
// entries left on the device; separate and aliased lists, a dropped list, the inertial tail; the scatter-back of the tracks read by the next
// frame; the capacity error as an exception.
#include <cstdio>
#include <cstdlib>

#include "local_map_synth.h"
#include "orbslam3_hip/Tracking.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using orbslam3_hip::LocalMap;

int main() {
    const int n_kf = 70, n_mp = 2500, n_feat = 220;
    localmap_synth::World W = localmap_synth::make(11, n_kf, n_mp, n_feat);
    localmap_synth::Rng R(12);
    LocalMap::MapView MV;
    MV.mapPoints = W.mp.data(); MV.nMapPoints = n_mp; MV.obsStart = W.obs_start.data(); MV.observations = W.obs.data();
    MV.nObservations = (int)W.obs.size(); MV.keyFrames = W.kf.data(); MV.nKeyFrames = n_kf; MV.keyFrameMapPoints = W.kf_mp.data();
    MV.nKeyFrameMapPointRows = (int)W.kf_mp.size(); MV.children = W.children.data(); MV.nChildren = (int)W.children.size();
    MV.keyFramesByOrder = W.order.data(); MV.tracks = W.track.data();
    LocalMap LM;
    LM.SetMap(MV);
    localmap_host::Scratch S;
    localmap_host::Result H;
    LocalMap::Result D;
    std::vector<orbm_map_point> mp;
    std::vector<orbm_track> trk;
    int total = 0;
    for (int f = 0; f < 5; f++) {
        const bool aliased = f % 2 == 0;
        std::vector<int32_t> vote = localmap_synth::frame_points(R, n_mp, f == 3 ? 0 : 150 + 40 * f), frame = localmap_synth::frame_points(R, n_mp, 130);
        std::vector<int32_t> dropped = localmap_synth::frame_points(R, n_mp, f == 1 ? 0 : 25);
        std::vector<int32_t> hv = vote, hf = frame;
        const orbm_localmap_frame F{f == 4 ? -1 : R.below(n_kf), f >= 2 ? ORBM_LM_INERTIAL : 0u};
        localmap_host::update(W.map(), F, hv.data(), (int)hv.size(), aliased ? hv.data() : hf.data(), aliased ? (int)hv.size() : (int)hf.size(),
                              dropped.data(), (int)dropped.size(), W.track.data(), S, H);
        LocalMap::FrameView FV;
        FV.lastKeyFrame = F.last_kf; FV.inertial = (F.flags & ORBM_LM_INERTIAL) != 0;
        FV.votePoints = vote.data(); FV.nVote = (int)vote.size();
        if (!aliased) { FV.framePoints = frame.data(); FV.nFrame = (int)frame.size(); }
        FV.droppedPoints = dropped.data(); FV.nDropped = (int)dropped.size();
        LM.Update(FV, D);
        CHECK(D.flags == 0 && H.flags == 0);
        CHECK(D.localKeyFrames == std::vector<int>(H.local_kf.begin(), H.local_kf.end()));
        CHECK(D.referenceKeyFrame == H.ref_kf && D.maxVotes == H.max_votes);
        CHECK(D.localMapPoints == std::vector<int>(H.local_src.begin(), H.local_src.end()));
        CHECK(vote == hv && (aliased || frame == hf));
        // the records and tracks left on the device for the projection
        const size_t n = H.local_src.size();
        mp.resize(n + 1); trk.resize(n + 1);
        int32_t nmp = -1;
        orbslam3_hip::detail::download(&nmp, LM.deviceLocalCount(), 4, nullptr);
        orbslam3_hip::detail::download(mp.data(), LM.deviceLocalMapPoints(), n * sizeof(orbm_map_point), nullptr);
        orbslam3_hip::detail::download(trk.data(), LM.deviceLocalTracks(), n * sizeof(orbm_track), nullptr);
        orbslam3_hip::detail::check(orb_stream_sync(nullptr), "sync");
        CHECK(nmp == (int)n && LM.localCapacity() == n_mp);
        CHECK(n == 0 || std::memcmp(mp.data(), H.local_mp.data(), n * sizeof(orbm_map_point)) == 0);
        CHECK(n == 0 || std::memcmp(trk.data(), H.track.data(), n * sizeof(orbm_track)) == 0);
        total += (int)n;
        // stand-in for the projection: every local track entry changes on the device, then goes back to the slab; the host slab follows
        for (size_t j = 0; j < n; j++) { trk[j].in_view = (int32_t)(j & 1); trk[j].proj_x = (float)(f * 10000 + (int)j); W.track[H.local_src[j]] = trk[j]; }
        orbslam3_hip::detail::check(orb_memcpy_h2d(LM.deviceLocalTracks(), trk.data(), n * sizeof(orbm_track), nullptr), "h2d");
        LM.StoreTracks();
    }
    CHECK(total > 3000);
    {   // capacities: one short of what the frame needs throws, and the result still reports what fitted
        std::vector<int32_t> vote = localmap_synth::frame_points(R, n_mp, 200), hv = vote;
        const orbm_localmap_frame F{-1, 0u};
        localmap_host::update(W.map(), F, hv.data(), 200, hv.data(), 200, nullptr, 0, W.track.data(), S, H);
        LocalMap::FrameView FV;
        FV.votePoints = vote.data(); FV.nVote = 200;
        bool threw = false;
        try { LM.Update(FV, D, 0, (int)H.local_src.size() - 1); } catch (const std::length_error&) { threw = true; }
        CHECK(threw && (D.flags & ORBM_LM_MP_OVERFLOW) && D.localMapPoints.size() == H.local_src.size() - 1);
        threw = false;
        try { LM.Update(FV, D, (int)H.local_kf.size() - 1, 0); } catch (const std::length_error&) { threw = true; }
        CHECK(threw && (D.flags & ORBM_LM_KF_OVERFLOW) && D.localMapPoints.empty() && D.localKeyFrames.size() == H.local_kf.size() - 1);
        LM.Update(FV, D, (int)H.local_kf.size(), (int)H.local_src.size());
        CHECK(D.flags == 0 && D.localMapPoints.size() == H.local_src.size());
        vote[3] = n_mp + 7;
        threw = false;
        try { LM.Update(FV, D); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw && vote[3] == -1);
        LocalMap none;
        threw = false;
        try { none.Update(FV, D); } catch (const std::logic_error&) { threw = true; }
        CHECK(threw);
    }
    std::printf("local_map_test OK\n");
    return 0;
}
