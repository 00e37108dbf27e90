// orbslam3_hip/Tracking.h — adapter for ORB_SLAM3::Tracking::UpdateLocalMap over liborbhip.so (include/orbhip.h "Local map"):
// UpdateLocalKeyFrames (Tracking.cc:3042-3244), UpdateLocalPoints (:2998-3036) and the marking loop of SearchLocalPoints (:2852-2872) on the
// device map.  Flattened views in; the key-frame list, pKFmax and the local points' indices out; the records and track entries of the local
// points stay on the device, where orbm_project_map_points(ORBM_PROJ_LOCAL_MAP) reads them (deviceLocalMapPoints(), deviceLocalCount(),
// deviceLocalTracks()).  What stays with the caller: the choice of the voting frame (:3050), IncreaseVisible, mmProjectPoints, and the
// MapPoint* / KeyFrame* bookkeeping on the returned indices.  The gather loop is shown in INTEGRATION.md "Tracking::UpdateLocalMap".
#ifndef ORBSLAM3_HIP_TRACKING_H
#define ORBSLAM3_HIP_TRACKING_H
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "detail/DeviceIO.h"

namespace orbslam3_hip {

class LocalMap {
public:
    // The map, flattened on the host (index spaces as in include/orbhip.h "Local map").
    struct MapView {
        const orbm_map_point* mapPoints = nullptr; int nMapPoints = 0;
        const int32_t* obsStart = nullptr;                       // nMapPoints + 1
        const orbm_observation* observations = nullptr; int nObservations = 0;
        const orbm_localmap_keyframe* keyFrames = nullptr; int nKeyFrames = 0;
        const int32_t* keyFrameMapPoints = nullptr; int nKeyFrameMapPointRows = 0;
        const int32_t* children = nullptr; int nChildren = 0;
        const int32_t* keyFramesByOrder = nullptr;               // nKeyFrames: the key-frame index at each rank of KeyFrame* order
        const orbm_track* tracks = nullptr;                      // nMapPoints, or nullptr = all zero (nothing in view yet)
    };
    // One frame's lists of map-point indices (-1 = none).  Bad points are nulled in place, as the reference nulls them.
    struct FrameView {
        int lastKeyFrame = -1;              // mCurrentFrame.mpLastKeyFrame
        bool inertial = false;              // mSensor is IMU_MONOCULAR or IMU_STEREO
        int32_t* votePoints = nullptr; int nVote = 0;     // mCurrentFrame.mvpMapPoints or mLastFrame.mvpMapPoints by the test at :3050
        int32_t* framePoints = nullptr; int nFrame = 0;   // mCurrentFrame.mvpMapPoints; nullptr = the vote list
        const int32_t* droppedPoints = nullptr; int nDropped = 0;   // the outliers an earlier step removed (:2234-2240, :2415)
    };
    struct Result {
        std::vector<int> localKeyFrames;    // mvpLocalKeyFrames
        int referenceKeyFrame = -1;         // pKFmax, or -1: keep mpReferenceKF
        int maxVotes = 0;
        std::vector<int> localMapPoints;    // mvpLocalMapPoints; record j on the device belongs to localMapPoints[j]
        uint32_t flags = 0;                 // ORBM_LM_* bits
    };

    // Uploads the map: for callers whose map lives on the host.  Synchronous.
    void SetMap(const MapView& M) {
        if (M.nMapPoints < 0 || M.nKeyFrames < 0 || M.nObservations < 0 || M.nKeyFrameMapPointRows < 0 || M.nChildren < 0 || !M.obsStart)
            throw std::invalid_argument("LocalMap: bad map view");
        std::memset(&view_, 0, sizeof view_);
        view_.d_mp = mp_.upload(M.mapPoints, (size_t)M.nMapPoints);
        view_.d_obs_start = obsStart_.upload(M.obsStart, (size_t)M.nMapPoints + 1);
        view_.d_obs = obs_.upload(M.observations, (size_t)M.nObservations);
        view_.d_kf = kf_.upload(M.keyFrames, (size_t)M.nKeyFrames);
        view_.d_kf_mp = kfMp_.upload(M.keyFrameMapPoints, (size_t)M.nKeyFrameMapPointRows);
        view_.d_children = children_.upload(M.children, (size_t)M.nChildren);
        view_.d_kf_by_order = order_.upload(M.keyFramesByOrder, (size_t)M.nKeyFrames);
        if (M.tracks) view_.d_mp_track = tracks_.upload(M.tracks, (size_t)M.nMapPoints);
        else {
            view_.d_mp_track = (orbm_track*)tracks_.ensure((size_t)M.nMapPoints * sizeof(orbm_track) + 16);
            detail::check(orb_memset(view_.d_mp_track, 0, (size_t)M.nMapPoints * sizeof(orbm_track), nullptr), "orb_memset");
        }
        view_.n_mp = M.nMapPoints; view_.n_obs = M.nObservations; view_.n_kf = M.nKeyFrames; view_.n_kf_mp_rows = M.nKeyFrameMapPointRows;
        view_.n_children = M.nChildren; view_.track_stride = 0;
        detail::check(orb_stream_sync(nullptr), "orb_stream_sync");
        haveMap_ = true;
    }
    // For callers whose map is on the device already (the slabs orbm_refresh_map_points / orbm_append_new_map_points keep current).
    void UseDeviceMap(const orbm_localmap_view& view) { view_ = view; view_.track_stride = 0; haveMap_ = true; }

    // One frame.  One upload (the frame record and the lists), the launches, one download (counts, flags, the two index lists, the nulled
    // lists), one synchronisation.  capKeyFrames / capMapPoints: the device capacities (0 = every key frame / every map point, which cannot
    // overflow).  Throws std::length_error where a list does not fit (nothing is truncated silently) and std::runtime_error where the device
    // flagged an index out of range; the result is filled in before either.
    void Update(const FrameView& F, Result& R, int capKeyFrames = 0, int capMapPoints = 0, void* stream = nullptr) {
        using namespace detail;
        if (!haveMap_) throw std::logic_error("LocalMap: no map");
        if (F.nVote < 0 || F.nFrame < 0 || F.nDropped < 0 || (F.nVote && !F.votePoints) || (F.nDropped && !F.droppedPoints))
            throw std::invalid_argument("LocalMap: bad frame view");
        const bool aliased = !F.framePoints || F.framePoints == F.votePoints;
        const int nFrame = aliased ? F.nVote : F.nFrame;
        capKf_ = capKeyFrames > 0 ? capKeyFrames : (view_.n_kf > 0 ? view_.n_kf : 1);
        capMp_ = capMapPoints > 0 ? capMapPoints : (view_.n_mp > 0 ? view_.n_mp : 1);
        const int capF = (F.nVote > nFrame ? F.nVote : nFrame) > 0 ? (F.nVote > nFrame ? F.nVote : nFrame) : 1;
        const int capD = F.nDropped > 0 ? F.nDropped : 1;
        // in: frame record, counts {vote, frame, dropped}, the lists; the lists are also downloaded (they come back nulled)
        Layout in;
        const auto sFrame = in.add<orbm_localmap_frame>(1);
        const auto sCounts = in.add<int32_t>(3);
        const auto sDropped = in.add<int32_t>(capD);
        const auto sVote = in.add<int32_t>(capF);
        const auto sFrameList = in.add<int32_t>(aliased ? 0 : capF);
        // out: counts {n_kf, n_kf_required, ref_kf, max_votes, nmp, nmp_required, flags}, the two index lists
        Layout out;
        const auto sHead = out.add<int32_t>(7);
        const auto sKf = out.add<int32_t>(capKf_);
        const auto sSrc = out.add<int32_t>(capMp_);
        uint8_t* st = stage_.ensure(in.size());
        std::memset(st, 0, in.size());
        orbm_localmap_frame fr;
        fr.last_kf = F.lastKeyFrame; fr.flags = F.inertial ? ORBM_LM_INERTIAL : 0u;
        const int32_t counts[3] = {F.nVote, nFrame, F.nDropped};
        put(stage_, sFrame, &fr, 1);
        put(stage_, sCounts, counts, 3);
        if (F.nDropped) put(stage_, sDropped, F.droppedPoints, (size_t)F.nDropped);
        if (F.nVote) put(stage_, sVote, F.votePoints, (size_t)F.nVote);
        if (!aliased && nFrame) put(stage_, sFrameList, F.framePoints, (size_t)nFrame);
        in_.ensure(in.size() + 16);
        out_.ensure(out.size() + 16);
        localMp_.ensure((size_t)capMp_ * sizeof(orbm_map_point) + 16);
        localTrack_.ensure((size_t)capMp_ * sizeof(orbm_track) + 16);
        work_.ensure(orbm_local_map_workspace_bytes(view_.n_kf, view_.n_mp, 1) + 16);
        check(orb_memcpy_h2d(in_.p, st, in.size(), stream), "orb_memcpy_h2d");
        orbm_localmap_lists L;
        const int32_t* dc = at(in_, sCounts);
        L.d_vote_mp = at(in_, sVote); L.d_n_vote = dc;
        L.d_frame_mp = aliased ? L.d_vote_mp : at(in_, sFrameList); L.d_n_frame = dc + 1;
        L.d_dropped_mp = F.nDropped ? at(in_, sDropped) : nullptr; L.d_n_dropped = F.nDropped ? dc + 2 : nullptr;
        L.cap_f = capF; L.cap_dropped = F.nDropped ? capD : 0;
        int32_t* dh = at(out_, sHead);
        orbm_localmap_out O;
        O.d_n_local_kf = dh; O.d_n_local_kf_required = dh + 1; O.d_ref_kf = dh + 2; O.d_max_votes = dh + 3; O.d_nmp = dh + 4;
        O.d_nmp_required = dh + 5; O.d_flags = (uint32_t*)(dh + 6);
        O.d_local_kf = at(out_, sKf); O.d_local_src = at(out_, sSrc);
        O.d_local_mp = (orbm_map_point*)localMp_.p; O.d_track = (orbm_track*)localTrack_.p;
        O.cap_kf = capKf_; O.cap_mp = capMp_;
        dSrc_ = O.d_local_src; dNmp_ = O.d_nmp;
        check(orbm_update_local_map(&view_, at(in_, sFrame), &L, 1, &O, work_.p, stream), "orbm_update_local_map");
        uint8_t* bk = back_.ensure(out.size() + in.size());
        download(bk, out_.p, out.size(), stream);
        download(bk + out.size(), (const uint8_t*)in_.p + sVote.offset, in.size() - sVote.offset, stream);
        check(orb_stream_sync(stream), "orb_stream_sync");
        const int32_t* h = downloaded(back_, sHead, 0);
        R.localKeyFrames.assign(downloaded(back_, sKf, 0), downloaded(back_, sKf, 0) + h[0]);
        R.referenceKeyFrame = h[2]; R.maxVotes = h[3];
        R.localMapPoints.assign(downloaded(back_, sSrc, 0), downloaded(back_, sSrc, 0) + h[4]);
        R.flags = (uint32_t)h[6];
        const uint8_t* lists = bk + out.size();
        if (F.nVote) std::memcpy(F.votePoints, lists, (size_t)F.nVote * 4);
        if (!aliased && nFrame) std::memcpy(F.framePoints, lists + (sFrameList.offset - sVote.offset), (size_t)nFrame * 4);
        if (h[1] > capKf_ || h[5] > capMp_) throw std::length_error("LocalMap: the local map does not fit the capacities");
        if (R.flags & ORBM_LM_BAD_INDEX) throw std::runtime_error("LocalMap: an index was out of range");
    }

    // The scatter-back after orbm_project_map_points has updated deviceLocalTracks(): the next frame reads the members isInFrustum left.
    void StoreTracks(void* stream = nullptr) {
        if (!dSrc_) throw std::logic_error("LocalMap: no frame");
        detail::check(orbm_store_local_tracks((const orbm_track*)localTrack_.p, dSrc_, dNmp_, capMp_, 1, view_.d_mp_track, 0, view_.n_mp, stream),
                      "orbm_store_local_tracks");
    }

    // d_mp, d_nmp, cap_mp and d_track of orbm_project_map_points(ORBM_PROJ_LOCAL_MAP) for the frame of the last Update()
    const orbm_map_point* deviceLocalMapPoints() const { return (const orbm_map_point*)localMp_.p; }
    const int32_t* deviceLocalCount() const { return dNmp_; }
    orbm_track* deviceLocalTracks() const { return (orbm_track*)localTrack_.p; }
    int localCapacity() const { return capMp_; }
    const orbm_localmap_view& deviceMap() const { return view_; }

private:
    orbm_localmap_view view_;
    bool haveMap_ = false;
    int capKf_ = 0, capMp_ = 0;
    const int32_t* dSrc_ = nullptr;
    const int32_t* dNmp_ = nullptr;
    detail::DevBuf mp_, obsStart_, obs_, kf_, kfMp_, children_, order_, tracks_, in_, out_, localMp_, localTrack_, work_;
    detail::HostBuf stage_, back_;
};

}  // namespace orbslam3_hip
#endif
