// orbslam3_hip/LocalMapping.h — adapter for the neighbour loop of ORB_SLAM3::LocalMapping::CreateNewMapPoints (LocalMapping.cc:566-906) over
// liborbhip.so (include/orbhip.h "New map points"): for every neighbour key frame SearchForTriangulation and then the triangulation loop
// (:651-904), on one stream, the current key frame's map-point flags carried from one neighbour to the next on the device, one download at the
// end.  What stays with the caller: neighbour selection, the baseline / median-depth skip (:586-604), ComputeF12 and the epipole (the
// ORBmatcher adapter's caller evaluates them already), and the `new MapPoint` / AddObservation / AddMapPoint bookkeeping on the returned
// (idx1, idx2, pos) lists.  The gather loop is shown in INTEGRATION.md "LocalMapping::CreateNewMapPoints".
// Below it, KeyFrameCulling: the adapter for LocalMapping::KeyFrameCulling (:1170-1322) over "Key-frame culling"; SearchInNeighbors over
// "Fusion in the neighbours"; ProcessNewKeyFrame and MapPointCulling over "New key frame".
#ifndef ORBSLAM3_HIP_LOCALMAPPING_H
#define ORBSLAM3_HIP_LOCALMAPPING_H
#include <cstdint>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "detail/DeviceIO.h"

namespace orbslam3_hip {

class NewMapPoints {
public:
    // One key frame, flattened: what SearchForTriangulation and the triangulation loop read of it.
    struct KeyFrameView {
        int N = 0;
        const orb_keypoint* keysUn = nullptr;     // mvKeysUn
        const orb_keypoint* keys = nullptr;       // mvKeys (UnprojectStereo); nullptr = the same as keysUn
        const uint8_t* descriptors = nullptr;     // mDescriptors, N x 32
        const float* uRight = nullptr;            // mvuRight, or nullptr for a monocular key frame
        const float* depth = nullptr;             // mvDepth (with uRight)
        const uint8_t* hasMapPoint = nullptr;     // GetMapPoint(i) != NULL
        std::vector<int32_t> nodeId, nodeStart, featIdx;   // mFeatVec as CSR (node ids ascending)
        float Rcw[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tcw[3] = {0, 0, 0}, Ow[3] = {0, 0, 0};   // GetRotation() row-major, GetTranslation(), GetCameraCenter()
        int cameraType = ORBM_CAM_PINHOLE;        // ORBM_CAM_PINHOLE or ORBM_CAM_KB8 (mpCamera->GetType())
        bool hasCamera2 = false;                  // mpCamera2 != NULL: a fisheye rig, refused
        int NLeft = -1;
        std::vector<float> cameraParameters;      // mpCamera->mvParameters: 4 (pinhole) or 8 (KannalaBrandt8) values
        float invfx = 0, invfy = 0, mb = 0, mbf = 0;
        std::vector<float> levelSigma2, scaleFactors;   // mvLevelSigma2, mvScaleFactors
        float scaleFactor = 1.2f;                 // mfScaleFactor
        int index = 0;                            // the key frame's index in the device map's key-frame tables (observation records)
        int descRow0 = 0;                         // the row of its feature 0 in the key-frame descriptor slab
    };
    struct Neighbour {
        const KeyFrameView* kf = nullptr;         // pKF2
        float F12[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // ComputeF12(mpCurrentKeyFrame, pKF2), row-major
        float ep[2] = {0, 0};                     // the epipole SearchForTriangulation computes (ORBmatcher.cc:1149-1152)
        bool obsKf2First = false;                 // mObservations (std::map<KeyFrame*, ...>) iterates pKF2 before the current key frame
    };
    // The points one neighbour created, in the order the reference creates them (ascending idx1).
    struct Created {
        bool searched = false;                    // false: the abort predicate fired before this neighbour
        std::vector<int> idx1, idx2, how;         // features of the current key frame / of the neighbour; ORBM_NEWPT_CREATED_*
        std::vector<float> pos;                   // 3 per point
        uint32_t pairFlags = 0;                   // ORBM_NEWPT_PAIR_*
    };

    // The orbm_newpt_camera of a key frame.  Host only.  Throws std::invalid_argument for a rig, a camera type outside the two, a parameter
    // count that does not fit the type, or more than 16 levels: the records are read on the device, which cannot refuse them.
    static orbm_newpt_camera BuildCamera(const KeyFrameView& K) {
        if (K.hasCamera2 || K.NLeft != -1) throw std::invalid_argument("NewMapPoints: fisheye rigs (mpCamera2) are not supported");
        if (K.cameraType != ORBM_CAM_PINHOLE && K.cameraType != ORBM_CAM_KB8) throw std::invalid_argument("NewMapPoints: unknown camera type");
        const size_t want = K.cameraType == ORBM_CAM_KB8 ? 8 : 4;
        if (K.cameraParameters.size() != want) throw std::invalid_argument("NewMapPoints: camera parameter count does not fit the camera type");
        if (K.levelSigma2.size() > 16 || K.scaleFactors.size() != K.levelSigma2.size()) throw std::invalid_argument("NewMapPoints: at most 16 levels");
        orbm_newpt_camera c;
        std::memset(&c, 0, sizeof c);
        std::memcpy(c.Rcw, K.Rcw, sizeof c.Rcw);
        std::memcpy(c.tcw, K.tcw, sizeof c.tcw);
        std::memcpy(c.Ow, K.Ow, sizeof c.Ow);
        c.camera_type = K.cameraType;
        for (size_t i = 0; i < want; i++) c.k[i] = K.cameraParameters[i];
        c.invfx = K.invfx; c.invfy = K.invfy; c.mb = K.mb; c.mbf = K.mbf;
        for (size_t i = 0; i < K.levelSigma2.size(); i++) { c.level_sigma2[i] = K.levelSigma2[i]; c.scale_factors[i] = K.scaleFactors[i]; }
        return c;
    }
    // The pair record of (current key frame, neighbour): LocalMapping.cc:541-562 and :631-646 once per pair.  Host only.
    static orbm_newpt_pair BuildPair(const KeyFrameView& K1, const KeyFrameView& K2, bool obsKf2First, bool bFarPoints, float thFarPoints) {
        orbm_newpt_pair P;
        std::memset(&P, 0, sizeof P);
        P.cam1 = BuildCamera(K1);
        P.cam2 = BuildCamera(K2);
        P.ratio_factor = 1.5f * K1.scaleFactor;
        P.far_points = bFarPoints ? 1 : 0;
        P.th_far_points = thFarPoints;
        P.kf1 = K1.index; P.kf2 = K2.index;
        P.obs_kf2_first = obsKf2First ? 1 : 0;
        P.desc_row0_1 = K1.descRow0; P.desc_row0_2 = K2.descRow0;
        return P;
    }

    // The neighbour loop.  For neighbour i: `i > 0 && checkNewKeyFrames()` ends the loop (LocalMapping.cc:569; the predicate is polled on the
    // host between the neighbours' launches, nothing waits for the device); then orbm_search_for_triangulation(bOnlyStereo = false, bCoarse)
    // and orbm_create_new_map_points on `stream`.  The current key frame's hasMapPoint flags live on the device for the whole loop, so a
    // feature that got a point from an earlier neighbour is skipped by the later searches.  One download at the end.
    // capNew: the most points one neighbour may create (default: every feature); a neighbour that needs more throws std::length_error after
    // the download (nothing is truncated silently).  A pair flagged ORBM_NEWPT_PAIR_BAD_INDEX throws std::runtime_error.
    // hasMapPoint1After (optional): the current key frame's flags after the loop, N entries.
    // Returns the number of neighbours processed.
    int Run(const KeyFrameView& K1, const std::vector<Neighbour>& neighbours, bool bCoarse, bool bFarPoints, float thFarPoints,
            const std::function<bool()>& checkNewKeyFrames, std::vector<Created>& created, int capNew = 0,
            std::vector<uint8_t>* hasMapPoint1After = nullptr, bool checkOrientation = false, void* stream = nullptr) {
        using namespace detail;
        const int nn = (int)neighbours.size();
        created.assign(nn, Created());
        if (hasMapPoint1After) hasMapPoint1After->assign(K1.hasMapPoint, K1.hasMapPoint + K1.N);
        if (nn == 0 || K1.N == 0) return 0;
        if (capNew <= 0) capNew = K1.N;
        // every record is built (and refused) before anything is launched; the host sources of the asynchronous uploads live until the
        // final synchronisation, and the second side's buffers get their largest size up front so that nothing is reallocated mid-loop
        std::vector<orbm_newpt_pair> pairs(nn);
        std::vector<orbm_tri_pair> tris(nn);
        counts_.assign(2 * (size_t)(nn + 1), 0);
        size_t maxN2 = 0, maxNodes2 = 0;
        for (int i = 0; i < nn; i++) {
            if (!neighbours[i].kf) throw std::invalid_argument("NewMapPoints: null neighbour");
            const KeyFrameView& K2 = *neighbours[i].kf;
            pairs[i] = BuildPair(K1, K2, neighbours[i].obsKf2First, bFarPoints, thFarPoints);
            orbm_tri_pair& T = tris[i];
            std::memset(&T, 0, sizeof T);
            std::memcpy(T.F12, neighbours[i].F12, sizeof T.F12);
            T.ep[0] = neighbours[i].ep[0]; T.ep[1] = neighbours[i].ep[1];
            std::memcpy(T.level_sigma2_2, pairs[i].cam2.level_sigma2, sizeof T.level_sigma2_2);
            std::memcpy(T.scale_factors_2, pairs[i].cam2.scale_factors, sizeof T.scale_factors_2);
            if ((size_t)K2.N > maxN2) maxN2 = (size_t)K2.N;
            if (K2.nodeId.size() > maxNodes2) maxNodes2 = K2.nodeId.size();
        }
        reserveSide(side_[1], maxN2, maxNodes2);
        triPair_.ensure((size_t)nn * sizeof(orbm_tri_pair) + 16);
        pair_.ensure((size_t)nn * sizeof(orbm_newpt_pair) + 16);
        match_.ensure((size_t)K1.N * 4 + 4);
        status_.ensure((size_t)K1.N);
        pointOf_.ensure(((size_t)K1.N + maxN2) * 4);
        // outputs of all neighbours in one block: [new | nnew, nrequired, flags] per neighbour, then the current key frame's flags
        Layout io;
        std::vector<Section<orbm_new_point>> NW(nn);
        std::vector<Section<int32_t>> CT(nn);
        for (int i = 0; i < nn; i++) { NW[i] = io.add<orbm_new_point>(capNew); CT[i] = io.add<int32_t>(3); }
        const auto H1 = io.add<uint8_t>(K1.N);
        out_.ensure(io.size());
        orbm_tri_side t1;
        orbm_newpt_side s1;
        uploadSide(0, K1, t1, s1, at(out_, H1), &counts_[0], stream);
        int done = 0;
        for (int i = 0; i < nn; i++) {
            if (i > 0 && checkNewKeyFrames && checkNewKeyFrames()) break;
            const KeyFrameView& K2 = *neighbours[i].kf;
            created[i].searched = true;
            done++;
            check(orb_memset(at(out_, CT[i]), 0, CT[i].bytes, stream), "orb_memset");
            if (K2.N == 0 || K1.nodeId.empty() || K2.nodeId.empty()) continue;   // SearchForTriangulation finds nothing
            orbm_tri_side t2;
            orbm_newpt_side s2;
            uploadSide(1, K2, t2, s2, nullptr, &counts_[2 * (size_t)(i + 1)], stream);
            orbm_tri_pair* dT = (orbm_tri_pair*)triPair_.p + i;
            orbm_newpt_pair* dP = (orbm_newpt_pair*)pair_.p + i;
            check(orb_memcpy_h2d(dT, &tris[i], sizeof tris[i], stream), "orb_memcpy_h2d");
            check(orb_memcpy_h2d(dP, &pairs[i], sizeof pairs[i], stream), "orb_memcpy_h2d");
            int32_t* dm = (int32_t*)match_.p;
            int32_t* dnm = dm + K1.N;
            check(orbm_search_for_triangulation(&t1, &t2, dT, 1, 0, bCoarse ? 1 : 0, checkOrientation ? 1 : 0, dm, dnm, stream),
                  "orbm_search_for_triangulation");
            uint8_t* dst = (uint8_t*)status_.p;
            int32_t* dp1 = (int32_t*)pointOf_.p;
            int32_t* dct = at(out_, CT[i]);
            check(orbm_create_new_map_points(&s1, &s2, dP, dm, 1, dst, at(out_, NW[i]), capNew, dct, dct + 1, dp1, dp1 + K1.N, (uint32_t*)(dct + 2),
                                             stream), "orbm_create_new_map_points");
        }
        download(back_.ensure(io.size()), out_.p, io.size(), stream);
        check(orb_stream_sync(stream), "orb_stream_sync");
        if (hasMapPoint1After) std::memcpy(hasMapPoint1After->data(), downloaded(back_, H1, 0), K1.N);
        for (int i = 0; i < nn; i++) {
            if (!created[i].searched) continue;
            const int32_t* ct = downloaded(back_, CT[i], 0);
            const orbm_new_point* np = downloaded(back_, NW[i], 0);
            Created& C = created[i];
            C.pairFlags = (uint32_t)ct[2];
            if (C.pairFlags & (ORBM_NEWPT_PAIR_BAD_INDEX | ORBM_NEWPT_PAIR_BAD_CAMERA)) throw std::runtime_error("NewMapPoints: a pair was flagged on the device");
            if (ct[1] > capNew) throw std::length_error("NewMapPoints: a neighbour created more points than capNew");
            for (int j = 0; j < ct[0]; j++) {
                C.idx1.push_back(np[j].idx1); C.idx2.push_back(np[j].idx2); C.how.push_back(np[j].how);
                C.pos.insert(C.pos.end(), np[j].pos, np[j].pos + 3);
            }
        }
        return done;
    }

private:
    struct SideBufs { detail::DevBuf kps, raw, desc, uRight, depth, hasMapPoint, nodeId, nodeStart, featIdx, counts; } side_[2];
    detail::DevBuf triPair_, pair_, match_, status_, pointOf_, out_;
    detail::HostBuf back_;
    std::vector<int32_t> counts_;   // per side {node count, N}: the host source of an asynchronous upload

    static void* upload(detail::DevBuf& b, const void* h, size_t bytes, void* stream) {
        void* d = b.ensure(bytes + 16);
        if (bytes) detail::check(orb_memcpy_h2d(d, h, bytes, stream), "orb_memcpy_h2d");
        return d;
    }
    // key frame K -> side i's buffers, as both kernels read it; hasMp: where the flags live (nullptr: the side's own buffer)
    static void reserveSide(SideBufs& B, size_t n, size_t nodes) {
        B.kps.ensure(n * sizeof(orb_keypoint) + 16); B.raw.ensure(n * sizeof(orb_keypoint) + 16); B.desc.ensure(n * 32 + 16);
        B.uRight.ensure(n * 4 + 16); B.depth.ensure(n * 4 + 16); B.hasMapPoint.ensure(n + 16); B.nodeId.ensure(nodes * 4 + 16);
        B.nodeStart.ensure(nodes * 4 + 20); B.featIdx.ensure(n * 4 + 16); B.counts.ensure(8 + 16);
    }
    void uploadSide(int i, const KeyFrameView& K, orbm_tri_side& t, orbm_newpt_side& s, uint8_t* hasMp, int32_t* counts, void* stream) {
        SideBufs& B = side_[i];
        counts[0] = (int32_t)K.nodeId.size(); counts[1] = K.N;
        const int32_t* dc = (const int32_t*)upload(B.counts, counts, 2 * sizeof(int32_t), stream);
        if (!hasMp) hasMp = (uint8_t*)B.hasMapPoint.ensure((size_t)K.N + 16);
        detail::check(orb_memcpy_h2d(hasMp, K.hasMapPoint, (size_t)K.N, stream), "orb_memcpy_h2d");
        t.kps = (const orb_keypoint*)upload(B.kps, K.keysUn, (size_t)K.N * sizeof(orb_keypoint), stream);
        t.desc = (const uint8_t*)upload(B.desc, K.descriptors, (size_t)K.N * 32, stream);
        t.u_right = K.uRight ? (const float*)upload(B.uRight, K.uRight, (size_t)K.N * 4, stream) : nullptr;
        t.has_mp = hasMp;
        t.node_id = (const int32_t*)upload(B.nodeId, K.nodeId.data(), K.nodeId.size() * 4, stream);
        t.node_start = (const int32_t*)upload(B.nodeStart, K.nodeStart.data(), K.nodeStart.size() * 4, stream);
        t.feat_idx = (const int32_t*)upload(B.featIdx, K.featIdx.data(), K.featIdx.size() * 4, stream);
        t.n_nodes = dc;
        t.cap_f = K.N; t.cap_nodes = (int32_t)K.nodeId.size();
        s.kps = t.kps;
        s.kps_raw = K.keys ? (const orb_keypoint*)upload(B.raw, K.keys, (size_t)K.N * sizeof(orb_keypoint), stream) : nullptr;
        s.u_right = t.u_right;
        s.depth = K.uRight ? (const float*)upload(B.depth, K.depth, (size_t)K.N * 4, stream) : nullptr;
        s.n = dc + 1;
        s.has_mp = hasMp;
        s.cap_f = K.N; s.reserved = 0;
    }
};

// Adapter for ORB_SLAM3::LocalMapping::KeyFrameCulling (LocalMapping.cc:1170-1322) over liborbhip.so (include/orbhip.h "Key-frame culling"):
// the redundancy walk over the local key frames on the device map, with the observation bookkeeping of KeyFrame::SetBadFlag.  Flattened views
// in; per candidate the exit code, nMPs and nRedundantObservations, and the ordered list of cull events out, in one download.  What stays
// with the caller: per event, in order, MergePrevious, the link updates and the spanning-tree work of KeyFrame::SetBadFlag.  The candidate list
// (GetVectorCovisibleKeyFrames) can be read from the device too: orbslam3_hip::CovisibilityGraph (KeyFrame.h) keeps the covisibility graph
// on this adapter's deviceMap(), and its EraseConnections folds the cull events into it.  The gather loop and the replay loop are shown in INTEGRATION.md
// "LocalMapping::KeyFrameCulling".
class KeyFrameCulling {
public:
    // The map, flattened on the host (index spaces as in include/orbhip.h "Local map" and "Key-frame culling").
    struct MapView {
        const orbm_map_point* mapPoints = nullptr; int nMapPoints = 0;
        const int32_t* obsStart = nullptr;                       // nMapPoints + 1
        const orbm_observation* observations = nullptr; int nObservations = 0;
        const orbm_localmap_keyframe* keyFrames = nullptr; int nKeyFrames = 0;
        const int32_t* keyFrameMapPoints = nullptr; int nKeyFrameMapPointRows = 0;
        const orbm_cull_keyframe* cullKeyFrames = nullptr;       // nKeyFrames
        const uint8_t* features = nullptr;                       // nKeyFrameMapPointRows: FeatureByte() of every feature
        const int32_t* mapPointObservations = nullptr;           // nMapPoints: MapPoint::nObs, or nullptr (the weighted sum over the records)
        bool hasRig = false;                                     // a key frame with NLeft != -1 or mpCamera2: refused
    };
    struct Settings {
        bool inertial = false, monocular = false;   // mbInertial, mbMonocular
        bool imuInitialized = false;                // mpAtlas->isImuInitialized()
        bool inertialBA2 = false;                   // mpCurrentKeyFrame->GetMap()->GetIniertialBA2()
        uint32_t initKeyFrameId = 0;                // GetMap()->GetInitKFid()
        int keyFramesInMap = 0;                     // mpAtlas->KeyFramesInMap()
    };
    struct Event { int keyFrame, prev, next; };     // prev / next: the links the inertial branch relinked, -1 / -1 otherwise
    struct Result {
        std::vector<uint8_t> codes;                 // ORBM_CULL_CODE_* per candidate
        std::vector<int> nMPs, nRedundantObservations;
        std::vector<Event> events;                  // one per KeyFrame::SetBadFlag call, in order
        uint32_t flags = 0;                         // ORBM_CULL_BAD_INDEX | ORBM_CULL_UNSUPPORTED
    };

    // The byte of one feature: mvKeysUn[i].octave, mvDepth[i] against mThDepth with the reference's expression, mvuRight[i].
    static uint8_t FeatureByte(int octave, float depth, float thDepth, float uRight) {
        if (octave < 0 || octave > (int)ORBM_CULL_FEAT_OCTAVE) throw std::invalid_argument("KeyFrameCulling: octave outside [0, 64)");
        const bool close = !(depth > thDepth || depth < 0);
        return (uint8_t)((unsigned)octave | (close ? ORBM_CULL_FEAT_CLOSE : 0u) | (uRight >= 0 ? ORBM_CULL_FEAT_STEREO : 0u));
    }

    // Uploads the map: for callers whose map lives on the host.  Synchronous.
    void SetMap(const MapView& M) {
        if (M.hasRig) throw std::invalid_argument("KeyFrameCulling: fisheye rigs (NLeft != -1, mpCamera2) are not supported");
        if (M.nMapPoints < 0 || M.nKeyFrames < 0 || M.nObservations < 0 || M.nKeyFrameMapPointRows < 0 || !M.obsStart ||
            (M.nKeyFrames && !M.cullKeyFrames) || (M.nKeyFrameMapPointRows && !M.features))
            throw std::invalid_argument("KeyFrameCulling: bad map view");
        std::memset(&view_, 0, sizeof view_);
        std::memset(&in_, 0, sizeof in_);
        view_.d_mp = mp_.upload(M.mapPoints, (size_t)M.nMapPoints);
        view_.d_obs_start = obsStart_.upload(M.obsStart, (size_t)M.nMapPoints + 1);
        view_.d_obs = obs_.upload(M.observations, (size_t)M.nObservations);
        view_.d_kf = kf_.upload(M.keyFrames, (size_t)M.nKeyFrames);
        view_.d_kf_mp = kfMp_.upload(M.keyFrameMapPoints, (size_t)M.nKeyFrameMapPointRows);
        in_.d_ckf = ckf_.upload(M.cullKeyFrames, (size_t)M.nKeyFrames);
        in_.d_feat = feat_.upload(M.features, (size_t)M.nKeyFrameMapPointRows);
        in_.d_mp_nobs = M.mapPointObservations ? nobs_.upload(M.mapPointObservations, (size_t)M.nMapPoints) : nullptr;
        view_.n_mp = M.nMapPoints; view_.n_obs = M.nObservations; view_.n_kf = M.nKeyFrames; view_.n_kf_mp_rows = M.nKeyFrameMapPointRows;
        detail::check(orb_stream_sync(nullptr), "orb_stream_sync");
        haveMap_ = true;
    }
    // For callers whose map is on the device already: the view of LocalMap plus the culling's own arrays (d_mp_nobs may be NULL).
    void UseDeviceMap(const orbm_localmap_view& view, const orbm_cull_keyframe* d_ckf, const uint8_t* d_feat, const int32_t* d_mp_nobs) {
        view_ = view;
        std::memset(&in_, 0, sizeof in_);
        in_.d_ckf = d_ckf; in_.d_feat = d_feat; in_.d_mp_nobs = d_mp_nobs;
        haveMap_ = true;
    }

    // One call of KeyFrameCulling.  current: mpCurrentKeyFrame; candidates: GetVectorCovisibleKeyFrames() in its order (key-frame indices);
    // pbAbortBA: &mbAbortBA, read ONCE here (the reference reads it at the bottom of every iteration; nullptr = false).  One upload (the
    // problem record and the candidates), the launches, one download, one synchronisation.  Throws std::runtime_error where the device met
    // an index out of range or a rig record; the result is filled in before.  The map itself is not changed: the outcome stays in
    // deviceWorkspace() for orbm_apply_keyframe_culling(deviceMap(), deviceInputs(), 1, 0, ...).
    void Run(int current, const std::vector<int>& candidates, const Settings& S, const bool* pbAbortBA, Result& R, void* stream = nullptr) {
        using namespace detail;
        if (!haveMap_) throw std::logic_error("KeyFrameCulling: no map");
        const int n = (int)candidates.size(), cap = n > 0 ? n : 1;
        Layout in;
        const auto sProblem = in.add<orbm_cull_problem>(1);
        const auto sCand = in.add<int32_t>(cap);
        Layout out;
        const auto sHead = out.add<int32_t>(2);   // n_events, flags
        const auto sCode = out.add<uint8_t>(cap);
        const auto sNmps = out.add<int32_t>(cap);
        const auto sNred = out.add<int32_t>(cap);
        const auto sEvents = out.add<orbm_cull_event>(cap);
        uint8_t* st = stage_.ensure(in.size());
        std::memset(st, 0, in.size());
        orbm_cull_problem P;
        P.current_kf = current; P.init_kf_id = S.initKeyFrameId; P.cand_start = 0; P.n_cand = n; P.n_kf_in_map = S.keyFramesInMap;
        P.flags = (S.inertial ? ORBM_CULL_INERTIAL : 0u) | (S.monocular ? ORBM_CULL_MONOCULAR : 0u) |
                  (S.imuInitialized ? ORBM_CULL_IMU_INITIALIZED : 0u) | (S.inertialBA2 ? ORBM_CULL_INERTIAL_BA2 : 0u) |
                  ((pbAbortBA && *pbAbortBA) ? ORBM_CULL_ABORT_BA : 0u);
        put(stage_, sProblem, &P, 1);
        std::vector<int32_t> c32(candidates.begin(), candidates.end());
        if (n) put(stage_, sCand, c32.data(), (size_t)n);
        inBuf_.ensure(in.size() + 16);
        outBuf_.ensure(out.size() + 16);
        work_.ensure(orbm_cull_workspace_bytes(view_.n_kf, view_.n_mp, view_.n_obs, 1) + 16);
        check(orb_memcpy_h2d(inBuf_.p, st, in.size(), stream), "orb_memcpy_h2d");
        in_.d_problems = at(inBuf_, sProblem); in_.d_candidates = at(inBuf_, sCand); in_.n_candidates = n; in_.n_cand_max = n;
        int32_t* dh = at(outBuf_, sHead);
        orbm_cull_out O;
        O.d_code = at(outBuf_, sCode); O.d_nmps = at(outBuf_, sNmps); O.d_nred = at(outBuf_, sNred); O.d_events = at(outBuf_, sEvents);
        O.d_n_events = dh; O.d_flags = (uint32_t*)(dh + 1); O.cap_cand = cap; O.reserved = 0;
        check(orbm_cull_keyframes(&view_, &in_, 1, &O, work_.p, stream), "orbm_cull_keyframes");
        download(back_.ensure(out.size()), outBuf_.p, out.size(), stream);
        check(orb_stream_sync(stream), "orb_stream_sync");
        const int32_t* h = downloaded(back_, sHead, 0);
        R.flags = (uint32_t)h[1];
        R.codes.assign(downloaded(back_, sCode, 0), downloaded(back_, sCode, 0) + n);
        R.nMPs.assign(downloaded(back_, sNmps, 0), downloaded(back_, sNmps, 0) + n);
        R.nRedundantObservations.assign(downloaded(back_, sNred, 0), downloaded(back_, sNred, 0) + n);
        R.events.clear();
        const orbm_cull_event* ev = downloaded(back_, sEvents, 0);
        for (int i = 0; i < h[0] && i < n; i++) R.events.push_back(Event{ev[i].kf, ev[i].prev, ev[i].next});
        if (R.flags & ORBM_CULL_BAD_INDEX) throw std::runtime_error("KeyFrameCulling: an index was out of range");
        if (R.flags & ORBM_CULL_UNSUPPORTED) throw std::runtime_error("KeyFrameCulling: the map holds a rig observation");
    }

    const orbm_localmap_view& deviceMap() const { return view_; }
    const orbm_cull_in& deviceInputs() const { return in_; }
    void* deviceWorkspace() const { return work_.p; }

private:
    orbm_localmap_view view_;
    orbm_cull_in in_;
    bool haveMap_ = false;
    detail::DevBuf mp_, obsStart_, obs_, kf_, kfMp_, ckf_, feat_, nobs_, inBuf_, outBuf_, work_;
    detail::HostBuf stage_, back_;
};

// Adapter for ORB_SLAM3::LocalMapping::SearchInNeighbors (LocalMapping.cc:913-1043) over liborbhip.so (include/orbhip.h "Fusion in the
// neighbours"): target selection, one ORBmatcher::Fuse per target, the candidates and the Fuse into the current key frame, with
// MapPoint::Replace / AddObservation folded into the device map.  Flattened records in; the ordered event list, the targets, mpReplaced, the
// current key frame's points and the merged observation rows out, in one download.  What stays with the caller: per event, in order, the
// pointer side of Replace / AddObservation (mpMap->EraseMapPoint and the rest), and the tail :1045-1065, which is
// orbm_refresh_map_points over Result::sel and CovisibilityGraph::UpdateConnections on deviceMap().  The gather and the replay loop are
// shown in INTEGRATION.md "LocalMapping::SearchInNeighbors".
class SearchInNeighbors {
public:
    // The map, flattened on the host: KeyFrameCulling::MapView's members and what Fuse reads beyond them.  The per-feature tables are
    // parallel to keyFrameMapPoints.
    struct MapView {
        KeyFrameCulling::MapView map;
        const orbm_fusenb_pose* poses = nullptr;                 // nKeyFrames
        const orb_keypoint* keyPoints = nullptr;                 // mvKeysUn of every key frame
        const float* uRight = nullptr;                           // mvuRight
        const uint8_t* keyFrameDescriptors = nullptr; int nKeyFrameDescriptorRows = 0;
        const uint8_t* mapPointDescriptors = nullptr; int nMapPointDescriptorRows = 0;   // GetDescriptor() of every point, row orbm_map_point.desc_row
        const int32_t* orderedKeyFrames = nullptr;               // [nKeyFrames][capConnections] mvpOrderedConnectedKeyFrames
        const int32_t* nOrdered = nullptr; int capConnections = 1;
        const int32_t* pointerOrder = nullptr;                   // nKeyFrames: key-frame indices sorted by KeyFrame* address
        const uint32_t* fuseTargets = nullptr;                   // nKeyFrames: mnFuseTargetForKF
        const int32_t* found = nullptr; const int32_t* visible = nullptr;   // nMapPoints: mnFound / mnVisible, or nullptr: not tracked
        int maxFeatures = 1;                                     // the greatest N of any key frame
        bool mixedSettings = false;                              // key frames of more than one camera or extractor setting: refused
    };
    struct Camera {
        float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0, th = 3.0f;
        float bounds[4] = {0, 0, 0, 0};                          // mnMinX, mnMaxX, mnMinY, mnMaxY
        orbm_grid_params grid = {0, 0, 0, 0};
        std::vector<float> scaleFactors, invLevelSigma2;         // mvScaleFactors, mvInvLevelSigma2
        float logScaleFactor = 0;                                // mfLogScaleFactor
    };
    struct Settings {
        bool monocular = false, inertial = false;                // mbMonocular, mbInertial
        // Capacities; 0 = derived from the map: every point can be a candidate, every feature row an event twice over, every row a new record.
        // capTargets sizes the chain of launches (7 per possible Fuse call, idle ones included): the targets expected, not the 420 possible.
        int capTargets = 40, capCandidates = 0, capEvents = 0, capObservations = 0;
    };
    struct Event { int call, keyFrame, listIndex, point, feature, other, kind; };   // kind: ORBM_FUSENB_EV_*
    struct Result {
        std::vector<int> targets, candidates, nFused;            // nFused[t] per target, nFused[targets.size()] for the Fuse into the current key frame
        std::vector<Event> events;
        std::vector<int> replaced, sel;                          // mpReplaced per point (-1: none); the current key frame's points after the fusion
        std::vector<int32_t> obsStart;                           // the merged rows (empty on ORBM_FUSENB_OBS_OVERFLOW)
        std::vector<orbm_observation> observations;
        int targetsRequired = 0, candidatesRequired = 0, observationsRequired = 0;
        uint32_t flags = 0;                                      // ORBM_FUSENB_* flag bits
    };

    void SetCamera(const Camera& C) {
        const size_t n = C.scaleFactors.size();
        if (n < 1 || n > 16 || C.invLevelSigma2.size() != n) throw std::invalid_argument("SearchInNeighbors: 1..16 levels, one inverse sigma2 per level");
        std::memset(&params_, 0, sizeof params_);
        params_.fx = C.fx; params_.fy = C.fy; params_.cx = C.cx; params_.cy = C.cy; params_.mbf = C.mbf; params_.th = C.th;
        std::memcpy(params_.bounds, C.bounds, sizeof params_.bounds);
        params_.grid = C.grid;
        params_.nlevels = (int32_t)n;
        for (size_t i = 0; i < n; i++) { params_.scale_factors[i] = C.scaleFactors[i]; params_.inv_level_sigma2[i] = C.invLevelSigma2[i]; }
        detail::check(orbm_predict_scale_thresholds(C.logScaleFactor, (int)n, params_.level_thresholds), "orbm_predict_scale_thresholds");
        haveCamera_ = true;
    }

    // Uploads the map: for callers whose map lives on the host.  Synchronous.
    void SetMap(const MapView& V) {
        const KeyFrameCulling::MapView& M = V.map;
        if (M.hasRig) throw std::invalid_argument("SearchInNeighbors: fisheye rigs (NLeft != -1, mpCamera2) are not supported");
        if (V.mixedSettings) throw std::invalid_argument("SearchInNeighbors: one camera and one extractor setting per map");
        if (M.nMapPoints < 0 || M.nKeyFrames < 0 || M.nObservations < 0 || M.nKeyFrameMapPointRows < 0 || !M.obsStart || V.capConnections < 1 ||
            V.maxFeatures < 1 || !V.keyFrameDescriptors || !V.mapPointDescriptors ||
            (M.nKeyFrames && (!M.cullKeyFrames || !V.poses || !V.orderedKeyFrames || !V.nOrdered || !V.pointerOrder || !V.fuseTargets)) ||
            (M.nKeyFrameMapPointRows && (!M.features || !V.keyPoints || !V.uRight)))
            throw std::invalid_argument("SearchInNeighbors: bad map view");
        const size_t nk = (size_t)M.nKeyFrames, nm = (size_t)M.nMapPoints, nr = (size_t)M.nKeyFrameMapPointRows;
        std::memset(&view_, 0, sizeof view_);
        std::memset(&in_, 0, sizeof in_);
        std::memset(&out_, 0, sizeof out_);
        out_.d_mp = mp_.upload(M.mapPoints, nm);
        view_.d_mp = out_.d_mp;
        view_.d_obs_start = obsStart_.upload(M.obsStart, nm + 1);
        view_.d_obs = obs_.upload(M.observations, (size_t)M.nObservations);
        view_.d_kf = kf_.upload(M.keyFrames, nk);
        out_.d_kf_mp = kfMp_.upload(M.keyFrameMapPoints, nr);
        view_.d_kf_mp = out_.d_kf_mp;
        view_.d_kf_by_order = order_.upload(V.pointerOrder, nk);
        view_.n_mp = M.nMapPoints; view_.n_obs = M.nObservations; view_.n_kf = M.nKeyFrames; view_.n_kf_mp_rows = M.nKeyFrameMapPointRows;
        in_.d_ckf = ckf_.upload(M.cullKeyFrames, nk);
        in_.d_pose = pose_.upload(V.poses, nk);
        in_.d_feat = feat_.upload(M.features, nr);
        in_.d_kps = kps_.upload(V.keyPoints, nr);
        in_.d_u_right = uRight_.upload(V.uRight, nr);
        in_.d_kf_desc = kfDesc_.upload(V.keyFrameDescriptors, (size_t)V.nKeyFrameDescriptorRows * 32);
        in_.d_ordered_kf = ordered_.upload(V.orderedKeyFrames, nk * (size_t)V.capConnections);
        in_.d_n_ordered = nOrdered_.upload(V.nOrdered, nk);
        out_.d_mp_nobs = M.mapPointObservations ? nobs_.upload(M.mapPointObservations, nm) : nullptr;
        in_.d_mp_nobs = out_.d_mp_nobs;
        in_.n_kf_desc_rows = V.nKeyFrameDescriptorRows; in_.cap_conn = V.capConnections; in_.cap_feat = V.maxFeatures;
        out_.d_found = V.found ? found_.upload(V.found, nm) : nullptr;
        out_.d_visible = V.visible ? visible_.upload(V.visible, nm) : nullptr;
        out_.d_mp_desc = mpDesc_.upload(V.mapPointDescriptors, (size_t)V.nMapPointDescriptorRows * 32);
        out_.n_desc_rows = V.nMapPointDescriptorRows;
        out_.d_fuse_target = targets_.upload(V.fuseTargets, nk);
        detail::check(orb_stream_sync(nullptr), "orb_stream_sync");
        haveMap_ = true;
    }

    // One call of SearchInNeighbors for key frame `current`.  pbAbortBA: &mbAbortBA, read ONCE here (nullptr = false).  The launches, one
    // download, one synchronisation.  The device map is folded in place (deviceMap(), deviceInputs(), deviceOutputs() name its slabs).
    // Throws std::runtime_error where the device met an index out of range or a rig record and std::length_error where a capacity did
    // not hold; the result is filled in before.
    void Run(int current, const Settings& settings, const bool* pbAbortBA, Result& R, void* stream = nullptr) {
        using namespace detail;
        if (!haveMap_ || !haveCamera_) throw std::logic_error("SearchInNeighbors: no map or no camera");
        Settings S = settings;
        if (S.capCandidates == 0) S.capCandidates = view_.n_mp > 0 ? view_.n_mp : 1;
        if (S.capEvents == 0) S.capEvents = 2 * view_.n_kf_mp_rows + 1;
        if (S.capObservations == 0) S.capObservations = view_.n_obs + view_.n_kf_mp_rows;
        if (S.capTargets < 1 || S.capTargets > ORBM_FUSENB_MAX_TARGETS || S.capCandidates < 1 || S.capEvents < 1 || S.capObservations < 0)
            throw std::invalid_argument("SearchInNeighbors: capacities");
        const size_t nm = (size_t)view_.n_mp;
        Layout out;
        const auto sResult = out.add<int32_t>(ORBM_FUSENB_R_WORDS);
        const auto sTargets = out.add<int32_t>((size_t)S.capTargets);
        const auto sCand = out.add<int32_t>((size_t)S.capCandidates);
        const auto sFused = out.add<int32_t>((size_t)S.capTargets + 1);
        const auto sEvents = out.add<orbm_fusenb_event>((size_t)S.capEvents);
        const auto sReplaced = out.add<int32_t>(nm);
        const auto sSel = out.add<int32_t>((size_t)in_.cap_feat);
        const auto sStart = out.add<int32_t>(nm + 1);
        const auto sObs = out.add<orbm_observation>((size_t)S.capObservations);
        outBuf_.ensure(out.size() + 16);
        const size_t wb = orbm_fusenb_workspace_bytes(view_.n_kf, view_.n_mp, view_.n_obs, in_.cap_feat, S.capCandidates, S.capEvents);
        if (!wb) throw std::invalid_argument("SearchInNeighbors: sizes");
        work_.ensure(wb + 16);
        orbm_fusenb_out O = out_;
        O.d_result = at(outBuf_, sResult); O.d_targets = at(outBuf_, sTargets); O.d_candidates = at(outBuf_, sCand); O.d_nfused = at(outBuf_, sFused);
        O.d_events = at(outBuf_, sEvents); O.d_replaced = at(outBuf_, sReplaced); O.d_sel = at(outBuf_, sSel);
        O.d_obs_start_out = at(outBuf_, sStart); O.d_obs_out = at(outBuf_, sObs);
        O.cap_targets = S.capTargets; O.cap_candidates = S.capCandidates; O.cap_events = S.capEvents; O.cap_obs_out = S.capObservations;
        orbm_fusenb_params P = params_;
        P.current_kf = current;
        P.flags = (S.monocular ? ORBM_FUSENB_MONOCULAR : 0u) | (S.inertial ? ORBM_FUSENB_INERTIAL : 0u) |
                  ((pbAbortBA && *pbAbortBA) ? ORBM_FUSENB_ABORT_BA : 0u);
        check(orbm_search_in_neighbors(&view_, &in_, &P, &O, work_.p, stream), "orbm_search_in_neighbors");
        download(back_.ensure(out.size()), outBuf_.p, out.size(), stream);
        check(orb_stream_sync(stream), "orb_stream_sync");
        const int32_t* h = downloaded(back_, sResult, 0);
        R.flags = (uint32_t)h[ORBM_FUSENB_R_FLAGS];
        R.targetsRequired = h[ORBM_FUSENB_R_N_TARGETS_REQUIRED]; R.candidatesRequired = h[ORBM_FUSENB_R_N_CANDIDATES_REQUIRED];
        R.observationsRequired = h[ORBM_FUSENB_R_N_OBS];
        const int nt = h[ORBM_FUSENB_R_N_TARGETS];
        R.targets.assign(downloaded(back_, sTargets, 0), downloaded(back_, sTargets, 0) + nt);
        R.candidates.assign(downloaded(back_, sCand, 0), downloaded(back_, sCand, 0) + h[ORBM_FUSENB_R_N_CANDIDATES]);
        R.nFused.assign(downloaded(back_, sFused, 0), downloaded(back_, sFused, 0) + S.capTargets + 1);
        R.events.clear();
        const orbm_fusenb_event* ev = downloaded(back_, sEvents, 0);
        for (int i = 0; i < h[ORBM_FUSENB_R_N_EVENTS]; i++)
            R.events.push_back(Event{ev[i].call, ev[i].kf, ev[i].list_index, ev[i].point, ev[i].feature, ev[i].other, ev[i].kind});
        R.replaced.assign(downloaded(back_, sReplaced, 0), downloaded(back_, sReplaced, 0) + nm);
        R.sel.assign(downloaded(back_, sSel, 0), downloaded(back_, sSel, 0) + h[ORBM_FUSENB_R_N_SEL]);
        R.obsStart.clear();
        R.observations.clear();
        if (!(R.flags & ORBM_FUSENB_OBS_OVERFLOW)) {
            R.obsStart.assign(downloaded(back_, sStart, 0), downloaded(back_, sStart, 0) + nm + 1);
            R.observations.assign(downloaded(back_, sObs, 0), downloaded(back_, sObs, 0) + h[ORBM_FUSENB_R_N_OBS]);
        }
        if (R.flags & ORBM_FUSENB_BAD_INDEX) throw std::runtime_error("SearchInNeighbors: an index was out of range");
        if (R.flags & ORBM_FUSENB_UNSUPPORTED) throw std::runtime_error("SearchInNeighbors: the map holds a rig observation");
        if (R.flags & (ORBM_FUSENB_TARGET_OVERFLOW | ORBM_FUSENB_CANDIDATE_OVERFLOW | ORBM_FUSENB_EVENT_OVERFLOW | ORBM_FUSENB_OBS_OVERFLOW |
                       ORBM_FUSENB_REFRESH_OVERFLOW))
            throw std::length_error("SearchInNeighbors: a capacity did not hold (Result::flags)");
    }

    const orbm_localmap_view& deviceMap() const { return view_; }
    const orbm_fusenb_in& deviceInputs() const { return in_; }
    const orbm_fusenb_out& deviceOutputs() const { return out_; }   // the in/out slabs: d_mp, d_kf_mp, d_mp_nobs, d_found, d_visible, d_mp_desc, d_fuse_target

private:
    orbm_localmap_view view_;
    orbm_fusenb_in in_;
    orbm_fusenb_out out_;
    orbm_fusenb_params params_;
    bool haveMap_ = false, haveCamera_ = false;
    detail::DevBuf mp_, obsStart_, obs_, kf_, kfMp_, order_, ckf_, pose_, feat_, kps_, uRight_, kfDesc_, ordered_, nOrdered_, nobs_, found_, visible_,
        mpDesc_, targets_, outBuf_, work_;
    detail::HostBuf back_;
};

// The device map of the two adapters below, and what their calls ping-pong: each call reads the CSR (and MapPointCulling the recent list) as
// it stands and writes the spare one, then the two change places.  An adapter hands its slabs to the other with
// other.UseDeviceMap(this.deviceSlabs()); the slabs stay owned by whoever uploaded them.
struct NewKeyFrameSlabs {
    orbm_localmap_view view;                                     // d_obs_start / d_obs / n_obs: the CSR as it stands
    orbm_newkf_in in;
    orbm_map_point* d_mp = nullptr;                              // the in/out slabs
    int32_t* d_kf_mp = nullptr;
    int32_t* d_mp_nobs = nullptr;                                // or nullptr: the weighted record sum
    uint8_t* d_mp_desc = nullptr; int nMapPointDescriptorRows = 0;
    int32_t* d_obs_start_spare = nullptr; orbm_observation* d_obs_spare = nullptr; int capObservations = 0;
    int32_t* d_recent = nullptr; int32_t* d_n_recent = nullptr;  // mlpRecentAddedMapPoints as it stands
    int32_t* d_recent_spare = nullptr; int32_t* d_n_recent_spare = nullptr; int capRecent = 1;
};

// What ProcessNewKeyFrame and MapPointCulling share: the map on the device.
class NewKeyFrameMap {
public:
    // The map, flattened on the host: KeyFrameCulling::MapView's members and what the two steps read beyond them.
    struct MapView {
        KeyFrameCulling::MapView map;
        const orbm_refresh_point* refPoints = nullptr;           // nMapPoints: mpRefKF and the reference key point's octave
        const orbm_keyframe_center* centers = nullptr;           // nKeyFrames: GetCameraCenter()
        const uint8_t* keyFrameDescriptors = nullptr; int nKeyFrameDescriptorRows = 0;
        const uint8_t* mapPointDescriptors = nullptr; int nMapPointDescriptorRows = 0;
        const int32_t* pointerOrder = nullptr;                   // nKeyFrames: key-frame indices sorted by KeyFrame* address
        const int32_t* found = nullptr; const int32_t* visible = nullptr;   // nMapPoints: mnFound / mnVisible
        const uint32_t* firstKeyFrameIds = nullptr;              // nMapPoints: mnFirstKFid
        std::vector<int> recent;                                 // mlpRecentAddedMapPoints
        int maxFeatures = 1;                                     // the greatest N the current key frame may have
        int capObservations = 0, capRecent = 0;                  // 0 = derived: a record more per feature row; the list twice over plus the rows
    };

    // Uploads the map: for callers whose map lives on the host.  Synchronous.
    void SetMap(const MapView& V) {
        const KeyFrameCulling::MapView& M = V.map;
        if (M.hasRig) throw std::invalid_argument("NewKeyFrameMap: fisheye rigs (NLeft != -1, mpCamera2) are not supported");
        if (M.nMapPoints < 0 || M.nKeyFrames < 0 || M.nObservations < 0 || M.nKeyFrameMapPointRows < 0 || !M.obsStart || V.maxFeatures < 1 ||
            V.capObservations < 0 || V.capRecent < 0 || !V.mapPointDescriptors || (M.nKeyFrames && (!M.cullKeyFrames || !V.centers || !V.pointerOrder)) ||
            (M.nKeyFrameMapPointRows && !M.features) || (M.nMapPoints && (!V.refPoints || !V.found || !V.visible || !V.firstKeyFrameIds)))
            throw std::invalid_argument("NewKeyFrameMap: bad map view");
        const size_t nk = (size_t)M.nKeyFrames, nm = (size_t)M.nMapPoints, nr = (size_t)M.nKeyFrameMapPointRows;
        const int capObs = V.capObservations ? V.capObservations : M.nObservations + M.nKeyFrameMapPointRows;
        const int capRecent = V.capRecent ? V.capRecent : 2 * (int)V.recent.size() + M.nKeyFrameMapPointRows + 1;
        if (capObs < M.nObservations || (size_t)capRecent < V.recent.size() || capRecent < 1) throw std::invalid_argument("NewKeyFrameMap: capacities");
        NewKeyFrameSlabs S;
        std::memset(&S.view, 0, sizeof S.view);
        std::memset(&S.in, 0, sizeof S.in);
        S.d_mp = mp_.upload(M.mapPoints, nm);
        S.view.d_mp = S.d_mp;
        int32_t* start = (int32_t*)obsStart_[0].ensure((nm + 1) * 4 + 16);
        orbm_observation* obs = (orbm_observation*)obs_[0].ensure((size_t)capObs * sizeof(orbm_observation) + 16);
        detail::check(orb_memcpy_h2d(start, M.obsStart, (nm + 1) * 4, nullptr), "orb_memcpy_h2d");
        if (M.nObservations) detail::check(orb_memcpy_h2d(obs, M.observations, (size_t)M.nObservations * sizeof(orbm_observation), nullptr), "orb_memcpy_h2d");
        S.view.d_obs_start = start; S.view.d_obs = obs;
        S.d_obs_start_spare = (int32_t*)obsStart_[1].ensure((nm + 1) * 4 + 16);
        S.d_obs_spare = (orbm_observation*)obs_[1].ensure((size_t)capObs * sizeof(orbm_observation) + 16);
        S.capObservations = capObs;
        S.view.d_kf = kf_.upload(M.keyFrames, nk);
        S.d_kf_mp = kfMp_.upload(M.keyFrameMapPoints, nr);
        S.view.d_kf_mp = S.d_kf_mp;
        S.view.d_kf_by_order = order_.upload(V.pointerOrder, nk);
        S.view.n_mp = M.nMapPoints; S.view.n_obs = M.nObservations; S.view.n_kf = M.nKeyFrames; S.view.n_kf_mp_rows = M.nKeyFrameMapPointRows;
        S.in.d_ckf = ckf_.upload(M.cullKeyFrames, nk);
        S.in.d_feat = feat_.upload(M.features, nr);
        S.in.d_ref = ref_.upload(V.refPoints, nm);
        S.in.d_center = center_.upload(V.centers, nk);
        S.in.d_kf_desc = kfDesc_.upload(V.keyFrameDescriptors, (size_t)V.nKeyFrameDescriptorRows * 32);
        S.in.d_found = found_.upload(V.found, nm);
        S.in.d_visible = visible_.upload(V.visible, nm);
        S.in.d_first_kf_id = first_.upload(V.firstKeyFrameIds, nm);
        S.in.n_kf_desc_rows = V.nKeyFrameDescriptorRows; S.in.cap_feat = V.maxFeatures;
        S.d_mp_nobs = M.mapPointObservations ? nobs_.upload(M.mapPointObservations, nm) : nullptr;
        S.d_mp_desc = mpDesc_.upload(V.mapPointDescriptors, (size_t)V.nMapPointDescriptorRows * 32);
        S.nMapPointDescriptorRows = V.nMapPointDescriptorRows;
        // the recent list: [entries | count] twice
        std::vector<int32_t> lst((size_t)capRecent + 4, -1);
        for (size_t i = 0; i < V.recent.size(); i++) lst[i] = V.recent[i];
        lst[(size_t)capRecent] = (int32_t)V.recent.size();
        S.d_recent = recent_[0].upload(lst.data(), lst.size());
        S.d_recent_spare = (int32_t*)recent_[1].ensure(lst.size() * 4 + 16);
        S.d_n_recent = S.d_recent + capRecent; S.d_n_recent_spare = S.d_recent_spare + capRecent;
        S.capRecent = capRecent;
        detail::check(orb_stream_sync(nullptr), "orb_stream_sync");
        slabs_ = S;
        haveMap_ = true;
    }
    // For callers whose map is on the device already, and for the hand-over between the two adapters.
    void UseDeviceMap(const NewKeyFrameSlabs& S) { slabs_ = S; haveMap_ = true; }
    const NewKeyFrameSlabs& deviceSlabs() const { return slabs_; }
    const orbm_localmap_view& deviceMap() const { return slabs_.view; }

    // mlpRecentAddedMapPoints.push_back of the points orbm_append_new_map_points made (its d_sel, n entries padded with -1), on `stream`.
    // Throws std::length_error where the list is full.
    void PushRecent(const int32_t* d_sel, int n, void* stream = nullptr) {
        using namespace detail;
        if (!haveMap_) throw std::logic_error("NewKeyFrameMap: no map");
        int32_t* d_res = (int32_t*)res_.ensure(ORBM_NEWKF_R_WORDS * 4 + 16);
        check(orbm_recent_points_push(d_sel, n, slabs_.d_recent, slabs_.d_n_recent, slabs_.capRecent, d_res, stream), "orbm_recent_points_push");
        int32_t h[ORBM_NEWKF_R_WORDS];
        download(h, d_res, sizeof h, stream);
        check(orb_stream_sync(stream), "orb_stream_sync");
        if (h[ORBM_NEWKF_R_FLAGS] & ORBM_NEWKF_BAD_INDEX) throw std::runtime_error("NewKeyFrameMap: the recent list's cursor was out of range");
        if (h[ORBM_NEWKF_R_FLAGS] & ORBM_NEWKF_RECENT_OVERFLOW) throw std::length_error("NewKeyFrameMap: the recent list is full");
    }

protected:
    NewKeyFrameSlabs slabs_;
    bool haveMap_ = false;
    detail::DevBuf outBuf_, work_;
    detail::HostBuf back_;
    static void throwOnFlags(uint32_t flags, const char* who) {
        if (flags & ORBM_NEWKF_BAD_INDEX) throw std::runtime_error(std::string(who) + ": an index was out of range");
        if (flags & ORBM_NEWKF_UNSUPPORTED) throw std::runtime_error(std::string(who) + ": the map holds a rig observation");
        if (flags & (ORBM_NEWKF_OBS_OVERFLOW | ORBM_NEWKF_RECENT_OVERFLOW | ORBM_NEWKF_REFRESH_OVERFLOW))
            throw std::length_error(std::string(who) + ": a capacity did not hold (Result::flags)");
    }
    void swapCsr(int nObs) {
        NewKeyFrameSlabs& S = slabs_;
        int32_t* s = const_cast<int32_t*>(S.view.d_obs_start);
        orbm_observation* o = const_cast<orbm_observation*>(S.view.d_obs);
        S.view.d_obs_start = S.d_obs_start_spare; S.view.d_obs = S.d_obs_spare; S.view.n_obs = nObs;
        S.d_obs_start_spare = s; S.d_obs_spare = o;
    }

private:
    detail::DevBuf mp_, obsStart_[2], obs_[2], kf_, kfMp_, order_, ckf_, feat_, ref_, center_, kfDesc_, found_, visible_, first_, nobs_, mpDesc_,
        recent_[2], res_;
};

// Adapter for the association loop of ORB_SLAM3::LocalMapping::ProcessNewKeyFrame (LocalMapping.cc:375-411) over liborbhip.so
// (include/orbhip.h "New key frame").  The caller has put the new key frame's own rows into the device map (or into the MapView).  What
// stays with the caller: ComputeBoW before, CovisibilityGraph::UpdateConnections on deviceMap() right after, mpAtlas->AddKeyFrame, and the
// pointer side of AddObservation for Result::added.  The binding is shown in INTEGRATION.md "LocalMapping::ProcessNewKeyFrame".
class ProcessNewKeyFrame : public NewKeyFrameMap {
public:
    struct Result {
        std::vector<uint8_t> codes;                 // ORBM_NEWKF_CODE_* per feature of the key frame's capacity
        std::vector<int> added;                     // the points that gained a record, in feature order
        int pushed = 0, pushesRequired = 0, observationsRequired = 0, recentSize = 0;
        uint32_t flags = 0;                         // ORBM_NEWKF_* flag bits
    };

    void SetScaleFactors(const std::vector<float>& scaleFactors) {   // mvScaleFactors
        if (scaleFactors.empty() || scaleFactors.size() > 16) throw std::invalid_argument("ProcessNewKeyFrame: 1..16 levels");
        std::memset(&params_, 0, sizeof params_);
        params_.what = ORBM_REFRESH_NORMAL_DEPTH | ORBM_REFRESH_DESCRIPTOR;
        params_.nlevels = (int32_t)scaleFactors.size();
        for (size_t i = 0; i < scaleFactors.size(); i++) params_.scale_factors[i] = scaleFactors[i];
        haveParams_ = true;
    }

    // One call for key frame `current`: the launches, one download (codes, selection, result words), one synchronisation.  The device map
    // is folded in place and the CSR slabs change places (deviceSlabs() names the merged one).  Throws std::runtime_error where the device
    // met an index out of range or a rig record and std::length_error where a capacity did not hold; the result is filled in before.
    void Run(int current, Result& R, void* stream = nullptr) {
        using namespace detail;
        if (!haveMap_ || !haveParams_) throw std::logic_error("ProcessNewKeyFrame: no map or no scale factors");
        NewKeyFrameSlabs& S = slabs_;
        const size_t cf = (size_t)S.in.cap_feat;
        Layout out;
        const auto sResult = out.add<int32_t>(ORBM_NEWKF_R_WORDS);
        const auto sRecentN = out.add<int32_t>(1);
        const auto sCode = out.add<uint8_t>(cf);
        const auto sSel = out.add<int32_t>(cf);
        outBuf_.ensure(out.size() + 16);
        const size_t wb = orbm_newkf_workspace_bytes(S.view.n_kf, S.view.n_mp, S.in.cap_feat);
        if (!wb) throw std::invalid_argument("ProcessNewKeyFrame: sizes");
        work_.ensure(wb + 16);
        orbm_newkf_out O;
        std::memset(&O, 0, sizeof O);
        O.d_mp = S.d_mp; O.d_mp_nobs = S.d_mp_nobs; O.d_mp_desc = S.d_mp_desc; O.d_code = at(outBuf_, sCode); O.d_sel = at(outBuf_, sSel);
        O.d_obs_start_out = S.d_obs_start_spare; O.d_obs_out = S.d_obs_spare; O.d_recent = S.d_recent; O.d_n_recent = S.d_n_recent;
        O.d_result = at(outBuf_, sResult);
        O.n_desc_rows = S.nMapPointDescriptorRows; O.cap_obs_out = S.capObservations; O.cap_recent = S.capRecent;
        check(orbm_process_new_keyframe(&S.view, &S.in, current, &params_, &O, work_.p, stream), "orbm_process_new_keyframe");
        check(orb_memcpy_d2h(back_.ensure(out.size()), outBuf_.p, out.size(), stream), "orb_memcpy_d2h");
        download(back_.p + sRecentN.offset, S.d_n_recent, 4, stream);
        check(orb_stream_sync(stream), "orb_stream_sync");
        const int32_t* h = downloaded(back_, sResult, 0);
        R.flags = (uint32_t)h[ORBM_NEWKF_R_FLAGS];
        R.pushed = h[ORBM_NEWKF_R_N_PUSHED]; R.pushesRequired = h[ORBM_NEWKF_R_N_PUSH_REQUIRED]; R.observationsRequired = h[ORBM_NEWKF_R_N_OBS];
        R.recentSize = *downloaded(back_, sRecentN, 0);
        R.codes.assign(downloaded(back_, sCode, 0), downloaded(back_, sCode, 0) + cf);
        R.added.clear();
        if (!(R.flags & ORBM_NEWKF_OBS_OVERFLOW)) {
            R.added.assign(downloaded(back_, sSel, 0), downloaded(back_, sSel, 0) + h[ORBM_NEWKF_R_N_ADDED]);
            swapCsr(h[ORBM_NEWKF_R_N_OBS]);
        }
        throwOnFlags(R.flags, "ProcessNewKeyFrame");
    }

private:
    orbm_refresh_params params_;
    bool haveParams_ = false;
};

// Adapter for ORB_SLAM3::LocalMapping::MapPointCulling (LocalMapping.cc:435-494) over liborbhip.so (include/orbhip.h "New key frame"), with
// the map effects of MapPoint::SetBadFlag folded into the device map.  What stays with the caller: mpMap->EraseMapPoint for Result::culled,
// in order.  The binding is shown in INTEGRATION.md "LocalMapping::MapPointCulling".
class MapPointCulling : public NewKeyFrameMap {
public:
    struct Result {
        std::vector<uint8_t> codes;                 // ORBM_MPCULL_CODE_* per list entry
        std::vector<int> culled, recent;            // the points SetBadFlag ran on, in list order; the surviving list
        int observationsRequired = 0;
        uint32_t flags = 0;                         // ORBM_NEWKF_* flag bits
    };

    // One call for key frame `current` (its id is nCurrentKFid): the launches, one download, one synchronisation.  The device map is folded
    // in place; the CSR slabs and the list slabs change places.  Exceptions as ProcessNewKeyFrame::Run.
    void Run(int current, bool monocular, Result& R, void* stream = nullptr) {
        using namespace detail;
        if (!haveMap_) throw std::logic_error("MapPointCulling: no map");
        NewKeyFrameSlabs& S = slabs_;
        const size_t cr = (size_t)S.capRecent;
        Layout out;
        const auto sResult = out.add<int32_t>(ORBM_NEWKF_R_WORDS);
        const auto sCode = out.add<uint8_t>(cr);
        const auto sCulled = out.add<int32_t>(cr);
        const auto sNCulled = out.add<int32_t>(1);
        const auto sRecent = out.add<int32_t>(cr);       // (a copy for the caller: the list itself stays on the device)
        outBuf_.ensure(out.size() + 16);
        const size_t wb = orbm_newkf_workspace_bytes(S.view.n_kf, S.view.n_mp, 1);
        if (!wb) throw std::invalid_argument("MapPointCulling: sizes");
        work_.ensure(wb + 16);
        orbm_mpcull_out O;
        std::memset(&O, 0, sizeof O);
        O.d_mp = S.d_mp; O.d_kf_mp = S.d_kf_mp; O.d_code = at(outBuf_, sCode); O.d_recent_out = S.d_recent_spare; O.d_n_recent_out = S.d_n_recent_spare;
        O.d_culled = at(outBuf_, sCulled); O.d_n_culled = at(outBuf_, sNCulled); O.d_obs_start_out = S.d_obs_start_spare; O.d_obs_out = S.d_obs_spare;
        O.d_result = at(outBuf_, sResult); O.cap_obs_out = S.capObservations; O.cap_recent = S.capRecent;
        check(orbm_cull_map_points(&S.view, &S.in, S.d_mp_nobs, current, monocular ? ORBM_MPCULL_MONOCULAR : 0u, S.d_recent, S.d_n_recent, &O,
                                   work_.p, stream), "orbm_cull_map_points");
        check(orb_memcpy_d2h(back_.ensure(out.size()), outBuf_.p, sRecent.offset, stream), "orb_memcpy_d2h");
        download(back_.p + sRecent.offset, S.d_recent_spare, cr * 4, stream);
        check(orb_stream_sync(stream), "orb_stream_sync");
        const int32_t* h = downloaded(back_, sResult, 0);
        R.flags = (uint32_t)h[ORBM_NEWKF_R_FLAGS];
        R.observationsRequired = h[ORBM_NEWKF_R_N_OBS];
        R.codes.assign(downloaded(back_, sCode, 0), downloaded(back_, sCode, 0) + h[ORBM_NEWKF_R_N_PUSH_REQUIRED]);
        R.culled.clear();
        R.recent.clear();
        if (!(R.flags & ORBM_NEWKF_OBS_OVERFLOW)) {
            R.culled.assign(downloaded(back_, sCulled, 0), downloaded(back_, sCulled, 0) + h[ORBM_NEWKF_R_N_ADDED]);
            R.recent.assign(downloaded(back_, sRecent, 0), downloaded(back_, sRecent, 0) + h[ORBM_NEWKF_R_N_PUSHED]);
            swapCsr(h[ORBM_NEWKF_R_N_OBS]);
            std::swap(S.d_recent, S.d_recent_spare);
            std::swap(S.d_n_recent, S.d_n_recent_spare);
        }
        throwOnFlags(R.flags, "MapPointCulling");
    }
};

}  // namespace orbslam3_hip
#endif
