// orbslam3_hip/ORBmatcher.h — adapter for ORB_SLAM3::ORBmatcher (reference include/ORBmatcher.h:39-94) over
// liborbhip.so (include/orbhip.h, stage 2).
//
// The reference methods take Frame& / KeyFrame* / MapPoint*; `FrameView` and `ProjectedPoint` are the flattened records an
// integration gathers from those objects (the gather loops are shown in INTEGRATION.md, one per call site) and
// `SearchByProjection*` scatter the result back in the reference's serial order (mvpMapPoints[idx] = pMP).
#ifndef ORBSLAM3_HIP_ORBMATCHER_H
#define ORBSLAM3_HIP_ORBMATCHER_H
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../orbhip.h"
#include "detail/DeviceIO.h"

namespace orbslam3_hip {

// What the matcher reads from an ORB_SLAM3::Frame (Nleft == -1): N, mvKeysUn, mDescriptors, mvuRight, and the static
// bounds mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv (Frame.cc:388-399).
struct FrameView {
    int N = 0;
    const orb_keypoint* keysUn = nullptr;     // == cv::KeyPoint array (28-byte layout)
    const uint8_t* descriptors = nullptr;     // N x 32
    const float* uRight = nullptr;            // mvuRight or nullptr (monocular)
    const uint8_t* occupied = nullptr;        // 1 where mvpMapPoints[i] && ->Observations()>0 before the call (or nullptr)
    orbm_grid_params grid{0, 0, 0, 0};
    // fisheye rig (Frame::Nleft != -1): keysUn / descriptors = [mvKeys | mvKeysRight] (N entries), Nleft as in the reference, kpLink[i] =
    // mvLeftToRightMatch[i] + Nleft for i < Nleft, mvRightToLeftMatch[i - Nleft] otherwise (or -1); queries then come as left/right twins
    // (ORBM_Q_RIGHT | ORBM_Q_TWIN, see orbhip.h)
    int Nleft = -1;
    const int32_t* kpLink = nullptr;
};

class ORBmatcher {
public:
    static const int TH_LOW = ORBM_TH_LOW, TH_HIGH = ORBM_TH_HIGH, HISTO_LENGTH = ORBM_HISTO_LENGTH;  // ORBmatcher.h:92-94

    ORBmatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}  // ORBmatcher.h:39

    // ORBmatcher::DescriptorDistance (ORBmatcher.cc:2700-2716).  A single 256-bit pair is not device work: this scalar
    // form serves one-off comparisons on the CPU; bulk distances go through orbm_hamming / the search kernels, and
    // MapPoint::ComputeDistinctiveDescriptors' pairwise distances through orbm_refresh_map_points (orbslam3_hip/MapPoint.h).
    static int DescriptorDistance(const uint8_t* a, const uint8_t* b) {
        int dist = 0;
        for (int i = 0; i < 8; i++) {
            uint32_t x, y;
            std::memcpy(&x, a + 4 * i, 4);
            std::memcpy(&y, b + 4 * i, 4);
            dist += __builtin_popcount(x ^ y);
        }
        return dist;
    }

    // Flattened SearchByProjection.  mode = ORBM_MODE_LOCAL_MAP  <=> SearchByProjection(Frame&, vector<MapPoint*>&, th, ...)  (ORBmatcher.cc:59)
    //                                mode = ORBM_MODE_BEST_ONLY  <=> SearchByProjection(Frame&, const Frame&, th, bMono)      (ORBmatcher.cc:2244)
    // queries[i]/qdesc[i] describe map point i (see orbm_query); kpMatch[idx] receives the index of the query whose map point
    // ends up in mvpMapPoints[idx] (-1: none).  Returns the reference's nmatches.
    int SearchByProjection(const FrameView& F, const std::vector<orbm_query>& queries, const std::vector<uint8_t>& qdesc, int mode,
                           int thDist, std::vector<int>& kpMatch, std::vector<int>& queryMatch) {
        const int n = F.N, nq = (int)queries.size();
        kpMatch.assign(n, -1);
        queryMatch.assign(nq, -1);
        if (n == 0 || nq == 0) return 0;
        // ONE packed host->device transfer per call: every input is laid out in a host staging block (256-byte aligned sections) that mirrors a
        // persistent device block; ONE device->host transfer brings back [q_match | kp_match | nmatches].  The buffers only ever grow.
        using namespace detail;
        const bool links = F.Nleft != -1 && F.kpLink;
        Layout in;
        const auto K = in.add<orb_keypoint>(n); const auto D = in.add<uint8_t>((size_t)n * 32); const auto U = in.add<float>(F.uRight ? n : 0);
        const auto O = in.add<uint8_t>(F.occupied ? n : 0); const auto Q = in.add<orbm_query>(nq); const auto QD = in.add<uint8_t>((size_t)nq * 32); const auto C = in.add<int32_t>(4);
        const auto L = in.add<int32_t>(links ? n : 0);
        stage_.ensure(in.size());
        put(stage_, K, F.keysUn, n);
        put(stage_, D, F.descriptors, (size_t)n * 32);
        if (F.uRight) put(stage_, U, F.uRight, n);
        if (F.occupied) put(stage_, O, F.occupied, n);
        put(stage_, Q, queries.data(), nq);
        put(stage_, QD, qdesc.data(), (size_t)nq * 32);
        const int32_t counts[3] = {n, nq, F.Nleft};
        put(stage_, C, counts, 3);
        if (links) put(stage_, L, F.kpLink, n);
        in_.upload(stage_.p, in.size());
        Layout out;
        const auto QM = out.add<int32_t>(nq); const auto KM = out.add<int32_t>(n); const auto NM = out.add<int32_t>(64);
        out_.ensure(out.size());
        const orb_keypoint* dk = at(in_, K);
        const uint8_t* docc = F.occupied ? at(in_, O) : nullptr;
        const int32_t* dc = at(in_, C);
        int32_t* gs = (int32_t*)gridStart_.ensure((2 * ORBM_GRID_COLS * ORBM_GRID_ROWS + 1) * 4);
        int32_t* gi = (int32_t*)gridIdx_.ensure((size_t)n * 4);
        void* work = work_.ensure(orbm_search_workspace_bytes(1, nq));
        orbm_search_params prm{mode, thDist, mfNNratio, mbCheckOrientation ? 1 : 0, F.grid};
        if (F.Nleft == -1) {
            check(orbm_grid_build(dk, dc, 1, n, 1, &F.grid, gs, gi, nullptr), "orbm_grid_build");
            check(orbm_search_by_projection(dk, at(in_, D), F.uRight ? at(in_, U) : nullptr, docc, dc, 1, n, gs, gi, at(in_, Q), at(in_, QD), dc + 1, nq, 1,
                                            &prm, at(out_, QM), at(out_, KM), at(out_, NM), work, nullptr), "orbm_search_by_projection");
        } else {
            check(orbm_grid_build_rig(dk, dc, dc + 2, 1, n, 1, &F.grid, gs, gi, nullptr), "orbm_grid_build_rig");
            check(orbm_search_by_projection_rig(dk, at(in_, D), docc, F.kpLink ? at(in_, L) : nullptr, dc, 1, n, gs, gi, at(in_, Q), at(in_, QD), dc + 1, nq,
                                                1, &prm, at(out_, QM), at(out_, KM), at(out_, NM), work, nullptr), "orbm_search_by_projection_rig");
        }
        const size_t len = NM.offset + 4;
        download(back_.ensure(len), out_.p, len, nullptr);
        check(orb_stream_sync(nullptr), "orb_stream_sync");
        std::memcpy(queryMatch.data(), downloaded(back_, QM, QM.offset), (size_t)nq * 4);
        std::memcpy(kpMatch.data(), downloaded(back_, KM, QM.offset), (size_t)n * 4);
        return *downloaded(back_, NM, QM.offset);
    }

    // ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORBmatcher.h:71, ORBmatcher.cc:838-979).
    // vbPrevMatched: x,y pairs per F1 keypoint, updated in place for the matched ones (:972-975).
    int SearchForInitialization(const FrameView& F1, const FrameView& F2, std::vector<float>& vbPrevMatched, std::vector<int>& vnMatches12,
                                int windowSize = 10) {
        std::vector<orbm_query> q(F1.N);
        for (int i = 0; i < F1.N; i++) {
            q[i] = orbm_query{vbPrevMatched[2 * i], vbPrevMatched[2 * i + 1], (float)windowSize, 0.f, F1.keysUn[i].angle, 0, 0,
                              F1.keysUn[i].octave == 0 ? ORBM_Q_VALID : 0u};
        }
        std::vector<uint8_t> qd(F1.descriptors, F1.descriptors + (size_t)F1.N * 32);
        std::vector<int> vnMatches21;
        const int n = SearchByProjection(F2, q, qd, ORBM_MODE_INIT, TH_LOW, vnMatches21, vnMatches12);
        for (int i = 0; i < F1.N; i++)
            if (vnMatches12[i] >= 0) { vbPrevMatched[2 * i] = F2.keysUn[vnMatches12[i]].x; vbPrevMatched[2 * i + 1] = F2.keysUn[vnMatches12[i]].y; }
        return n;
    }

    // The search half of ORBmatcher::Fuse (ORBmatcher.h:85-88).  The caller computes per map point what the reference computes before
    // KeyFrame::GetFeaturesInArea (uv, ur, radius = th*mvScaleFactors[nPredictedLevel], levels [nPredictedLevel-1, nPredictedLevel];
    // flags = ORBM_Q_VALID iff the point passed the gates of ORBmatcher.cc:1700-1765 / :1910-1955) and afterwards applies
    // Replace / AddObservation / vpReplacePoint in index order on bestIdx[i] >= 0 (ORBmatcher.cc:1832-1855 / :1987-2000).
    // invLevelSigma2 != nullptr selects the KeyFrame overload's chi2 gate (:1791-1815); nullptr = the Sim3 overload.
    int Fuse(const FrameView& KF, const std::vector<orbm_query>& queries, const std::vector<uint8_t>& qdesc, const float* invLevelSigma2,
             int nLevels, std::vector<int>& bestIdx, std::vector<int>& bestDist) {
        const int n = KF.N, nq = (int)queries.size();
        bestIdx.assign(nq, -1);
        bestDist.assign(nq, 256);
        if (n == 0 || nq == 0) return 0;
        using namespace detail;
        const orb_keypoint* dk = kps_.upload(KF.keysUn, n);
        const uint8_t* dd = desc_.upload(KF.descriptors, (size_t)n * 32);
        const float* dur = KF.uRight ? uRight_.upload(KF.uRight, n) : nullptr;
        const orbm_query* dq = queries_.upload(queries.data(), nq);
        const uint8_t* dqd = qdesc_.upload(qdesc.data(), (size_t)nq * 32);
        int32_t counts[2] = {n, nq};
        const int32_t* dc = counts_.upload(counts, 2);
        int32_t* gs = (int32_t*)gridStart_.ensure((ORBM_GRID_COLS * ORBM_GRID_ROWS + 1) * 4);
        int32_t* gi = (int32_t*)gridIdx_.ensure((size_t)n * 4);
        int32_t* dqm = (int32_t*)match_.ensure((size_t)nq * 4);
        int32_t* dqdist = (int32_t*)dist_.ensure((size_t)nq * 4);
        int32_t* dnm = (int32_t*)nMatches_.ensure(4);
        check(orbm_grid_build(dk, dc, 1, n, 1, &KF.grid, gs, gi, nullptr), "orbm_grid_build");
        orbm_fuse_params prm{};
        prm.th_dist = TH_LOW; prm.chi2_gate = invLevelSigma2 ? 1 : 0; prm.grid = KF.grid;
        for (int i = 0; i < 16 && i < nLevels && invLevelSigma2; i++) prm.inv_level_sigma2[i] = invLevelSigma2[i];
        check(orbm_fuse(dk, dd, dur, dc, 1, n, gs, gi, dq, dqd, dc + 1, nq, 1, &prm, dqm, dqdist, dnm, nullptr), "orbm_fuse");
        download(bestDist.data(), dqdist, (size_t)nq * 4, nullptr);
        return downloadMatches(bestIdx.data(), dqm, nq, dnm);
    }

    // ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (ORBmatcher.h:79, ORBmatcher.cc:2008-2220).  q12[i1] = the values the
    // reference computes for key frame 1's map point i1 before pKF2->GetFeaturesInArea (:2044-2080: VALID iff it exists, is not in vpMatches12
    // already, is not bad and passed the depth / image / distance gates; u, v, radius = th*mvScaleFactors[nPredictedLevel], max_level =
    // nPredictedLevel), q21[i2] likewise for key frame 2 (:2122-2158); the descriptors are pMP->GetDescriptor().  matches12[i1] = index into key
    // frame 2 of the agreed match or -1 (the caller sets vpMatches12[i1] = vpMapPoints2[idx2]); returns nFound.
    int SearchBySim3(const FrameView& KF1, const FrameView& KF2, const std::vector<orbm_query>& q12, const std::vector<uint8_t>& q12desc,
                     const std::vector<orbm_query>& q21, const std::vector<uint8_t>& q21desc, std::vector<int>& matches12) {
        const int n1 = KF1.N, n2 = KF2.N;
        matches12.assign(n1, -1);
        if ((int)q12.size() != n1 || (int)q21.size() != n2 || q12desc.size() != (size_t)n1 * 32 || q21desc.size() != (size_t)n2 * 32)
            throw std::invalid_argument("SearchBySim3: one query (and one 32-byte descriptor) per keypoint of each key frame is required");
        if (n1 == 0 || n2 == 0) return 0;
        using namespace detail;
        const int32_t counts[2] = {n1, n2};
        const int32_t* dc = counts_.upload(counts, 2);
        int32_t* vn1 = (int32_t*)match_.ensure((size_t)n1 * 4);
        int32_t* vn2 = (int32_t*)match2_.ensure((size_t)n2 * 4);
        int32_t* dist = (int32_t*)dist_.ensure((size_t)std::max(n1, n2) * 4);
        int32_t* dnm = (int32_t*)nMatches_.ensure(8);
        orbm_fuse_params prm{};
        prm.th_dist = TH_HIGH; prm.chi2_gate = 0;
        for (int dir = 0; dir < 2; dir++) {      // dir 0: key frame 1's points searched in key frame 2
            const FrameView& T = dir == 0 ? KF2 : KF1;
            const std::vector<orbm_query>& q = dir == 0 ? q12 : q21;
            const std::vector<uint8_t>& qd = dir == 0 ? q12desc : q21desc;
            const orb_keypoint* dk = kps_.upload(T.keysUn, T.N);
            const uint8_t* dd = desc_.upload(T.descriptors, (size_t)T.N * 32);
            const orbm_query* dq = queries_.upload(q.data(), q.size());
            const uint8_t* dqd = qdesc_.upload(qd.data(), qd.size());
            int32_t* gs = (int32_t*)gridStart_.ensure((ORBM_GRID_COLS * ORBM_GRID_ROWS + 1) * 4);
            int32_t* gi = (int32_t*)gridIdx_.ensure((size_t)T.N * 4);
            prm.grid = T.grid;
            check(orbm_grid_build(dk, dc + (dir == 0 ? 1 : 0), 1, T.N, 1, &T.grid, gs, gi, nullptr), "orbm_grid_build");
            check(orbm_fuse(dk, dd, nullptr, dc + (dir == 0 ? 1 : 0), 1, T.N, gs, gi, dq, dqd, dc + (dir == 0 ? 0 : 1), (int)q.size(), 1, &prm,
                            dir == 0 ? vn1 : vn2, dist, dnm, nullptr), "orbm_fuse");
            check(orb_stream_sync(nullptr), "orb_stream_sync");   // the upload buffers are reused by the second direction
        }
        int32_t* out = (int32_t*)mutual_.ensure((size_t)n1 * 4);
        check(orbm_mutual_matches(vn1, vn2, dc, dc + 1, n1, n2, 1, out, dnm + 1, nullptr), "orbm_mutual_matches");
        return downloadMatches(matches12.data(), out, n1, dnm + 1);
    }

    // One key frame as SearchForTriangulation reads it: mvKeysUn, mDescriptors, mvuRight, GetMapPoint(i) != NULL, and mFeatVec as CSR
    // (node ids ascending = std::map order; featIdx = the concatenated per-node index vectors).
    struct KeyFrameView {
        int N = 0;
        const orb_keypoint* keysUn = nullptr;
        const uint8_t* descriptors = nullptr;
        const float* uRight = nullptr;
        const uint8_t* hasMapPoint = nullptr;
        std::vector<int32_t> nodeId, nodeStart, featIdx;
    };
    // ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) (ORBmatcher.h:74, ORBmatcher.cc:1138-1428)
    // for pinhole key frames without mpCamera2.  F12: row-major K1^-T [t12]x R12 K2^-1 (the expression of Pinhole.cpp:157-160, evaluated
    // by the caller with the same cv::Mat arithmetic); ep: pKF2->mpCamera->project(R2w*Cw+t2w) (:1149-1152).
    int SearchForTriangulation(const KeyFrameView& K1, const KeyFrameView& K2, const float F12[9], const float ep[2], const float* levelSigma2_2,
                               const float* scaleFactors_2, int nLevels, std::vector<std::pair<size_t, size_t>>& vMatchedPairs, bool bOnlyStereo,
                               bool bCoarse = false) {
        vMatchedPairs.clear();
        if (K1.N == 0 || K2.N == 0 || K1.nodeId.empty() || K2.nodeId.empty()) return 0;
        using namespace detail;
        const int32_t nn[2] = {(int32_t)K1.nodeId.size(), (int32_t)K2.nodeId.size()};
        const int32_t* dnn = counts_.upload(nn, 2);
        const orbm_tri_side s[2] = {uploadTriSide(0, K1, dnn, true), uploadTriSide(1, K2, dnn + 1, true)};
        orbm_tri_pair P{};
        for (int i = 0; i < 9; i++) P.F12[i] = F12[i];
        P.ep[0] = ep[0]; P.ep[1] = ep[1];
        for (int i = 0; i < 16 && i < nLevels; i++) { P.level_sigma2_2[i] = levelSigma2_2[i]; P.scale_factors_2[i] = scaleFactors_2[i]; }
        const orbm_tri_pair* dP = pair_.upload(&P, 1);
        int32_t* dm = (int32_t*)match_.ensure((size_t)K1.N * 4);
        int32_t* dnm = (int32_t*)nMatches_.ensure(4);
        check(orbm_search_for_triangulation(&s[0], &s[1], dP, 1, bOnlyStereo ? 1 : 0, bCoarse ? 1 : 0, mbCheckOrientation ? 1 : 0, dm, dnm, nullptr), "orbm_search_for_triangulation");
        return downloadPairs(dm, dnm, K1.N, vMatchedPairs);
    }

    // The same call for key frames with KannalaBrandt8 cameras — a fisheye rig (pKF->mpCamera2 != NULL: K.keysUn = [mvKeys | mvKeysRight],
    // nLeft = pKF->NLeft) or one fisheye camera (nLeft = -1).  `pair` carries what the reference computes before its loops (ORBmatcher.cc:1144-1193):
    // the four (R12, t12) combinations, both cameras' parameters, the epipole and the level tables; see orbm_tri_kb8_pair in orbhip.h.
    int SearchForTriangulationKB8(const KeyFrameView& K1, int nLeft1, const KeyFrameView& K2, int nLeft2, const orbm_tri_kb8_pair& pair,
                                  std::vector<std::pair<size_t, size_t>>& vMatchedPairs, bool bOnlyStereo, bool bCoarse = false) {
        vMatchedPairs.clear();
        if (K1.N == 0 || K2.N == 0 || K1.nodeId.empty() || K2.nodeId.empty()) return 0;
        using namespace detail;
        const int32_t nn[4] = {(int32_t)K1.nodeId.size(), (int32_t)K2.nodeId.size(), nLeft1, nLeft2};
        const int32_t* dnn = counts_.upload(nn, 4);
        const orbm_tri_side s[2] = {uploadTriSide(0, K1, dnn, false), uploadTriSide(1, K2, dnn + 1, false)};
        const orbm_tri_kb8_pair* dP = pair_.upload(&pair, 1);
        int32_t* dm = (int32_t*)match_.ensure((size_t)K1.N * 4);
        int32_t* dnm = (int32_t*)nMatches_.ensure(4);
        check(orbm_search_for_triangulation_kb8(&s[0], &s[1], dnn + 2, dnn + 3, dP, 1, bOnlyStereo ? 1 : 0, bCoarse ? 1 : 0, mbCheckOrientation ? 1 : 0, dm,
                                                dnm, nullptr), "orbm_search_for_triangulation_kb8");
        return downloadPairs(dm, dnm, K1.N, vMatchedPairs);
    }

    // ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) (ORBmatcher.h:67, ORBmatcher.cc:323-587).
    // KF / F as KeyFrameView (descriptors + mFeatVec CSR; hasMapPoint on the KF side = "pKF map point exists and is not bad");
    // angleKF / angleF = keypoint angles (mvKeysUn / mvKeys / mvKeysRight as the reference picks them); nLeftF = F.Nleft (-1: one camera).
    // fMatch[j] = index of the KF feature whose map point lands in vpMapPointMatches[j], or -1.
    int SearchByBoW(const KeyFrameView& KF, const float* angleKF, const KeyFrameView& F, const float* angleF, int nLeftF, std::vector<int>& fMatch) {
        fMatch.assign(F.N, -1);
        if (KF.N == 0 || F.N == 0 || KF.nodeId.empty() || F.nodeId.empty()) return 0;
        using namespace detail;
        const int32_t nn[3] = {(int32_t)KF.nodeId.size(), (int32_t)F.nodeId.size(), nLeftF};
        const int32_t* dnn = counts_.upload(nn, 3);
        const orbm_bow_side s[2] = {uploadBowSide(0, KF, dnn, angleKF, nullptr), uploadBowSide(1, F, dnn + 1, angleF, nLeftF != -1 ? dnn + 2 : nullptr)};
        const uint8_t* dv = side_[0].hasMapPoint.upload(KF.hasMapPoint, KF.N);
        int32_t* dm = (int32_t*)match_.ensure((size_t)F.N * 4);
        int32_t* dnm = (int32_t*)nMatches_.ensure(4);
        check(orbm_search_by_bow(&s[0], dv, &s[1], 1, mfNNratio, mbCheckOrientation ? 1 : 0, dm, dnm, nullptr), "orbm_search_by_bow");
        return downloadMatches(fMatch.data(), dm, F.N, dnm);
    }

    // ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (ORBmatcher.h:68, ORBmatcher.cc:984-1124; call site
    // LoopClosing.cc:697).  K1 / K2 as KeyFrameView; hasMapPoint[i] = "GetMapPointMatches()[i] exists and is not bad" AND, for a fisheye-rig
    // key frame (NLeft != -1), i < mvKeysUn.size() (:1020-1022, :1043-1045).  matches12[i1] = index of the pKF2 feature whose map point
    // vpMatches12[i1] receives, or -1.
    int SearchByBoW(const KeyFrameView& K1, const float* angle1, const KeyFrameView& K2, const float* angle2, std::vector<int>& matches12) {
        matches12.assign(K1.N, -1);
        if (K1.N == 0 || K2.N == 0 || K1.nodeId.empty() || K2.nodeId.empty()) return 0;
        using namespace detail;
        const int32_t nn[2] = {(int32_t)K1.nodeId.size(), (int32_t)K2.nodeId.size()};
        const int32_t* dnn = counts_.upload(nn, 2);
        const orbm_bow_side s[2] = {uploadBowSide(0, K1, dnn, angle1, nullptr), uploadBowSide(1, K2, dnn + 1, angle2, nullptr)};
        const uint8_t* dv[2] = {side_[0].hasMapPoint.upload(K1.hasMapPoint, K1.N), side_[1].hasMapPoint.upload(K2.hasMapPoint, K2.N)};
        int32_t* dm = (int32_t*)match_.ensure((size_t)K1.N * 4);
        int32_t* dnm = (int32_t*)nMatches_.ensure(4);
        check(orbm_search_by_bow_kf(&s[0], dv[0], &s[1], dv[1], 1, mfNNratio, mbCheckOrientation ? 1 : 0, dm, dnm, nullptr), "orbm_search_by_bow_kf");
        return downloadMatches(matches12.data(), dm, K1.N, dnm);
    }

    // Projection and search on the device (orbm_project_map_points, then orbm_search_by_projection): the map points as host records
    // (desc_row indexes mpDesc, nDescRows x 32 bytes), the current pose (and the last frame's, LAST_FRAME) as an orbm_project_frame, the mode
    // and its parameters in prm (level_thresholds from orbm_predict_scale_thresholds).  The search mode follows the projection: LOCAL_MAP ->
    // ORBM_MODE_LOCAL_MAP, LAST_FRAME / RELOC -> ORBM_MODE_BEST_ONLY; thDist = TH_HIGH, or ORBdist for RELOC.  F.occupied holds the skip rule
    // of the search at hand, as for SearchByProjection.  LOCAL_MAP reads and updates track (one entry per map point: the mTrack* members).
    // kpMatch[idx] = index into mapPoints of the point mvpMapPoints[idx] holds after the call (-1: untouched, -2: set to NULL by the
    // orientation cull).  One packed upload, one packed download.  Returns nmatches (0 when LOCAL_MAP finds no point in view).
    int SearchByProjectionFromMap(const FrameView& F, const std::vector<orbm_map_point>& mapPoints, const uint8_t* mpDesc, int nDescRows,
                                  const orbm_project_frame& pose, const orbm_project_params& prm, int thDist, std::vector<orbm_track>& track,
                                  std::vector<int>& kpMatch) {
        const int n = F.N, nmp = (int)mapPoints.size();
        const bool localMap = prm.mode == ORBM_PROJ_LOCAL_MAP;
        kpMatch.assign(n, -1);
        if (F.Nleft != -1) throw std::invalid_argument("SearchByProjectionFromMap: single-camera frames only");
        if (localMap && (int)track.size() != nmp) throw std::invalid_argument("SearchByProjectionFromMap: one track entry per map point");
        if (nmp == 0) return 0;
        const int capK = std::max(n, 1), capQ = nmp;
        // one device block: the inputs, the track states, the downloaded outputs, then scratch; upload [0, TR + track), download [TR, NM + 16)
        using namespace detail;
        Layout io;
        const auto K = io.add<orb_keypoint>(capK); const auto D = io.add<uint8_t>((size_t)capK * 32); const auto U = io.add<float>(F.uRight ? n : 0);
        const auto O = io.add<uint8_t>(F.occupied ? n : 0); const auto MP = io.add<orbm_map_point>(nmp); const auto MD = io.add<uint8_t>((size_t)std::max(nDescRows, 1) * 32);
        const auto FR = io.add<orbm_project_frame>(1); const auto C = io.add<int32_t>(4); const auto TR = io.add<orbm_track>(nmp);
        const size_t upEnd = TR.offset + (localMap ? TR.bytes : 0);
        const auto KM = io.add<int32_t>(capK); const auto QS = io.add<int32_t>(capQ); const auto NM = io.add<int32_t>(4); const auto Q = io.add<orbm_query>(capQ);
        const auto QD = io.add<uint8_t>((size_t)capQ * 32); const auto QM = io.add<int32_t>(capQ);
        stage_.ensure(upEnd);
        if (n) {
            put(stage_, K, F.keysUn, n);
            put(stage_, D, F.descriptors, (size_t)n * 32);
        }
        if (F.uRight) put(stage_, U, F.uRight, n);
        if (F.occupied) put(stage_, O, F.occupied, n);
        put(stage_, MP, mapPoints.data(), nmp);
        if (nDescRows > 0) put(stage_, MD, mpDesc, (size_t)nDescRows * 32);
        put(stage_, FR, &pose, 1);
        const int32_t counts[2] = {n, nmp};
        put(stage_, C, counts, 2);
        if (localMap) put(stage_, TR, track.data(), nmp);
        io_.ensure(io.size());
        check(orb_memcpy_h2d(io_.p, stage_.p, upEnd, nullptr), "orb_memcpy_h2d");
        const int32_t* dc = at(io_, C);
        int32_t* nm = at(io_, NM);   // nmatches, nq, n_required, n_in_view
        orbm_project_params p = prm;
        p.n_desc_rows = nDescRows;
        check(orbm_project_map_points(at(io_, MP), dc + 1, capQ, at(io_, MD), at(io_, FR), 1, &p, localMap ? at(io_, TR) : nullptr, at(io_, Q), at(io_, QD),
                                      nm + 1, at(io_, QS), nm + 2, nm + 3, capQ, nullptr), "orbm_project_map_points");
        if (n) {
            int32_t* gs = (int32_t*)gridStart_.ensure((ORBM_GRID_COLS * ORBM_GRID_ROWS + 1) * 4);
            int32_t* gi = (int32_t*)gridIdx_.ensure((size_t)n * 4);
            void* work = work_.ensure(orbm_search_workspace_bytes(1, capQ));
            const orbm_search_params sp{localMap ? ORBM_MODE_LOCAL_MAP : ORBM_MODE_BEST_ONLY, thDist, mfNNratio, mbCheckOrientation ? 1 : 0, F.grid};
            check(orbm_grid_build(at(io_, K), dc, 1, n, 1, &F.grid, gs, gi, nullptr), "orbm_grid_build");
            check(orbm_search_by_projection(at(io_, K), at(io_, D), F.uRight ? at(io_, U) : nullptr, F.occupied ? at(io_, O) : nullptr, dc, 1, n, gs, gi,
                                            at(io_, Q), at(io_, QD), nm + 1, capQ, 1, &sp, at(io_, QM), at(io_, KM), nm, work, nullptr), "orbm_search_by_projection");
        } else {
            check(orb_memset(nm, 0, 4, nullptr), "orb_memset");
        }
        const size_t downLen = NM.offset + 16 - TR.offset;
        download(back_.ensure(downLen), at(io_, TR), downLen, nullptr);
        check(orb_stream_sync(nullptr), "orb_memcpy_d2h");
        if (localMap) std::memcpy(track.data(), downloaded(back_, TR, TR.offset), TR.bytes);
        const int32_t* km = downloaded(back_, KM, TR.offset);
        const int32_t* qs = downloaded(back_, QS, TR.offset);
        for (int i = 0; i < n; i++) kpMatch[i] = km[i] >= 0 ? qs[km[i]] : km[i];
        return *downloaded(back_, NM, TR.offset);
    }

    float mfNNratio;
    bool mbCheckOrientation;

private:
    // desc and the FeatureVector CSR of K -> side i's buffers: the fields orbm_tri_side and orbm_bow_side share (dNodes: K's node count on the device)
    template <class Side> void uploadSide(int i, const KeyFrameView& K, const int32_t* dNodes, Side& s) {
        s.desc = side_[i].desc.upload(K.descriptors, (size_t)K.N * 32);
        s.node_id = side_[i].nodeId.upload(K.nodeId.data(), K.nodeId.size());
        s.node_start = side_[i].nodeStart.upload(K.nodeStart.data(), K.nodeStart.size());
        s.feat_idx = side_[i].featIdx.upload(K.featIdx.data(), K.featIdx.size());
        s.n_nodes = dNodes;
        s.cap_f = K.N; s.cap_nodes = (int32_t)K.nodeId.size();
    }
    orbm_tri_side uploadTriSide(int i, const KeyFrameView& K, const int32_t* dNodes, bool stereo) {
        orbm_tri_side s;
        uploadSide(i, K, dNodes, s);
        s.kps = side_[i].kps.upload(K.keysUn, K.N);
        s.u_right = stereo && K.uRight ? side_[i].uRight.upload(K.uRight, K.N) : nullptr;
        s.has_mp = side_[i].hasMapPoint.upload(K.hasMapPoint, K.N);
        return s;
    }
    orbm_bow_side uploadBowSide(int i, const KeyFrameView& K, const int32_t* dNodes, const float* angle, const int32_t* dNleft) {
        orbm_bow_side s;
        uploadSide(i, K, dNodes, s);
        s.angle = side_[i].angle.upload(angle, K.N);
        s.n_left = dNleft;
        return s;
    }
    // the match index per feature and the match count -> the host; returns the count
    int downloadMatches(int* match, const int32_t* dMatch, int n, const int32_t* dCount) {
        int count = 0;
        detail::download(match, dMatch, (size_t)n * 4, nullptr);
        detail::download(&count, dCount, 4, nullptr);
        detail::check(orb_stream_sync(nullptr), "orb_stream_sync");
        return count;
    }
    // the same for the triangulation searches: match12 -> vMatchedPairs (ORBmatcher.cc:1415-1422)
    int downloadPairs(const int32_t* dm, const int32_t* dnm, int n1, std::vector<std::pair<size_t, size_t>>& vMatchedPairs) {
        std::vector<int> m12(n1);
        const int nmatches = downloadMatches(m12.data(), dm, n1, dnm);
        for (int i = 0; i < n1; i++)
            if (m12[i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)m12[i]));
        return nmatches;
    }

    detail::DevBuf in_, out_, io_;   // the packed blocks: SearchByProjection's input and output, SearchByProjectionFromMap's one block
    detail::HostBuf stage_, back_;   // their page-locked host mirrors
    detail::DevBuf kps_, desc_, uRight_, queries_, qdesc_;   // Fuse / SearchBySim3: the per-call inputs, one upload each
    struct SideBufs { detail::DevBuf kps, desc, uRight, hasMapPoint, angle, nodeId, nodeStart, featIdx; } side_[2];   // the two key-frame sides
    detail::DevBuf pair_, counts_;         // orbm_tri_pair / orbm_tri_kb8_pair; the few int32 every search reads: feature / query / node counts, Nleft
    detail::DevBuf gridStart_, gridIdx_, work_;   // orbm_grid_build's cell table and feature list; orbm_search_workspace_bytes
    // outputs: the match per query / feature, its distance (Fuse, SearchBySim3), SearchBySim3's second direction and agreed matches, the counters
    detail::DevBuf match_, dist_, match2_, mutual_, nMatches_;
};

}  // namespace orbslam3_hip
#endif
