// orbslam3_hip/TwoViewReconstruction.h — adapter for ORB_SLAM3::TwoViewReconstruction (reference include/TwoViewReconstruction.h,
// src/TwoViewReconstruction.cc) over liborbhip.so (include/orbhip.h "TwoViewReconstruction"): the geometric solver of
// Tracking::MonocularInitialization, between SearchForInitialization and CreateInitialMapMonocular, on the Pinhole path.
//
// The reference's constructor and Reconstruct() signatures, with the conventions of Sim3Solver.h for cv::Mat: K is 9 floats row-major, R21 is
// 9 floats row-major and t21 3 floats, both EMPTY where the reference leaves cv::Mat().  The key-point and point types are template
// parameters: anything with `.pt.x / .pt.y` (cv::KeyPoint) and `.x / .y / .z` (cv::Point3f).
//
// How it differs from the reference, and why the answers do not:
//  * mvSets are drawn as the reference draws them (:100-127): DUtils::Random::SeedRandOnce(0), then eight RandomInt per iteration on the
//    global rand() with the swap-with-back removal.  SeedRandOnce here has its own once-flag: a program that also links DUtils should call
//    DUtils::Random::SeedRandOnce(0) first and construct with seedRandOnce = false, so that rand() is seeded exactly once as in the reference.
//  * With fewer than 8 matches the reference draws from an empty range (undefined); this returns false without drawing or launching.
//  * FindHomography and FindFundamental are not two host threads but one launch over all 2 x mMaxIterations hypotheses.
#ifndef ORBSLAM3_HIP_TWOVIEWRECONSTRUCTION_H
#define ORBSLAM3_HIP_TWOVIEWRECONSTRUCTION_H
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "detail/DeviceIO.h"

namespace orbslam3_hip {

class TwoViewReconstruction {
public:
    // K: the 3x3 calibration matrix, row-major (fx, fy, cx, cy are read)
    TwoViewReconstruction(const std::vector<float>& K, float sigma = 1.0, int iterations = 200, void* stream = nullptr, bool seedRandOnce = true)
        : mSigma(sigma), mMaxIterations(iterations), stream_(stream), seed_(seedRandOnce) {
        if (K.size() != 9) throw std::invalid_argument("TwoViewReconstruction: K is 9 floats, row-major");
        if (iterations < 1) throw std::invalid_argument("TwoViewReconstruction: iterations below 1");
        fx_ = K[0]; fy_ = K[4]; cx_ = K[2]; cy_ = K[5];
    }

    // Reconstruct (:51-171).  vP3D and vbTriangulated get vKeys1.size() entries when it returns true and are left alone otherwise.
    template <class KeyPointT, class Point3T>
    bool Reconstruct(const std::vector<KeyPointT>& vKeys1, const std::vector<KeyPointT>& vKeys2, const std::vector<int>& vMatches12,
                     std::vector<float>& R21, std::vector<float>& t21, std::vector<Point3T>& vP3D, std::vector<bool>& vbTriangulated) {
        const int n1 = (int)vKeys1.size(), n2 = (int)vKeys2.size();
        R21.clear(); t21.clear();
        if ((int)vMatches12.size() != n1) throw std::invalid_argument("TwoViewReconstruction: vMatches12 has one entry per key of frame 1");
        int N = 0;
        for (int m : vMatches12) N += m >= 0;
        if (!Draw(N)) return false;
        const int cap_k = Cap(n1, n2);
        std::vector<orb_keypoint> k1((size_t)cap_k, orb_keypoint{}), k2((size_t)cap_k, orb_keypoint{});
        std::vector<int32_t> m12((size_t)cap_k, -1);
        for (int i = 0; i < n1; i++) { k1[i].x = vKeys1[i].pt.x; k1[i].y = vKeys1[i].pt.y; m12[i] = vMatches12[i]; }
        for (int i = 0; i < n2; i++) { k2[i].x = vKeys2[i].pt.x; k2[i].y = vKeys2[i].pt.y; }
        using namespace detail;
        Layout in;
        const auto K1 = in.add<orb_keypoint>(cap_k); const auto K2 = in.add<orb_keypoint>(cap_k); const auto M = in.add<int32_t>(cap_k);
        stage_in_.ensure(in.size());
        put(stage_in_, K1, k1.data(), k1.size());
        put(stage_in_, K2, k2.data(), k2.size());
        put(stage_in_, M, m12.data(), m12.size());
        keys_.ensure(in.size());
        check(orb_memcpy_h2d(keys_.p, stage_in_.p, in.size(), stream_), "orb_memcpy_h2d");
        if (!Run(at(keys_, K1), n1, at(keys_, K2), n2, at(keys_, M), R21, t21)) return false;
        vP3D.assign((size_t)n1, Point3T());
        vbTriangulated.assign((size_t)n1, false);
        for (int i = 0; i < n1; i++) {
            vP3D[i].x = p3d_[(size_t)i * 3]; vP3D[i].y = p3d_[(size_t)i * 3 + 1]; vP3D[i].z = p3d_[(size_t)i * 3 + 2];
            vbTriangulated[i] = tri_[i] != 0;
        }
        return true;
    }

    // The same on frames that stay on the device: d_keys1 [n1] / d_keys2 [n2] the undistorted records, d_matches12 [n1] what ORBM_MODE_INIT
    // wrote, nMatches its count of entries >= 0 (the host needs it to draw the sets).  vP3D: 3 floats per key of frame 1; vbTriangulated:
    // one byte per key.
    bool Reconstruct(const orb_keypoint* d_keys1, int n1, const orb_keypoint* d_keys2, int n2, const int32_t* d_matches12, int nMatches,
                     std::vector<float>& R21, std::vector<float>& t21, std::vector<float>& vP3D, std::vector<uint8_t>& vbTriangulated) {
        R21.clear(); t21.clear();
        if (!Draw(nMatches)) return false;
        if (!Run(d_keys1, n1, d_keys2, n2, d_matches12, R21, t21)) return false;
        vP3D.assign(p3d_.begin(), p3d_.begin() + (size_t)n1 * 3);
        vbTriangulated.assign(tri_.begin(), tri_.begin() + n1);
        return true;
    }

    // what the last launch produced
    const orbm_tvr_result& DeviceResult() const { return result_; }
    const std::vector<int32_t>& Sets() const { return sets_; }   // [mMaxIterations][8]

    // DUtils::Random::RandomInt(min, max) (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) and SeedRandOnce (:38-44)
    static int RandomInt(int min, int max) {
        const int d = max - min + 1;
        return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
    }
    static void SeedRandOnce(int seed) {
        static bool already = false;
        if (!already) { srand(seed); already = true; }
    }

private:
    static int Cap(int n1, int n2) { const int m = n1 > n2 ? n1 : n2; return m > 0 ? m : 1; }

    // mvSets (:100-127); false = fewer than 8 matches
    bool Draw(int N) {
        result_ = orbm_tvr_result{};
        if (N < 8) { result_.status = ORBM_TVR_TOO_FEW; result_.model = -1; result_.hypothesis = -1; return false; }
        sets_.assign((size_t)mMaxIterations * 8, 0);
        if (seed_) SeedRandOnce(0);
        std::vector<int32_t> avail;
        for (int it = 0; it < mMaxIterations; it++) {
            avail.resize(N);
            for (int i = 0; i < N; i++) avail[i] = i;   // vAvailableIndices = vAllIndices
            for (int j = 0; j < 8; j++) {
                const int randi = RandomInt(0, (int)avail.size() - 1);
                sets_[(size_t)it * 8 + j] = avail[randi];
                avail[randi] = avail.back();
                avail.pop_back();
            }
        }
        return true;
    }

    bool Run(const orb_keypoint* d_keys1, int n1, const orb_keypoint* d_keys2, int n2, const int32_t* d_matches12, std::vector<float>& R21,
             std::vector<float>& t21) {
        const int its = mMaxIterations, cap_k = Cap(n1, n2), words = (cap_k + 63) / 64;
        orbm_tvr_problem P{};
        P.fx = fx_; P.fy = fy_; P.cx = cx_; P.cy = cy_; P.sigma = mSigma; P.max_its = its; P.n_keys1 = n1; P.n_keys2 = n2;
        P.min_parallax = 1.0f; P.min_triangulated = 50;   // :157, :164 / :169
        // one device block: [problem | sets || result | p3d | triangulated || score | model | mask | work]; upload [0, R), download [R, S)
        using namespace detail;
        Layout io;
        const auto Pb = io.add<orbm_tvr_problem>(1); const auto Sets = io.add<int32_t>((size_t)its * 8); const auto R = io.add<orbm_tvr_result>(1);
        const auto X = io.add<float>((size_t)cap_k * 3); const auto T = io.add<uint8_t>(cap_k); const auto S = io.add<float>((size_t)2 * its);
        const auto Mo = io.add<float>((size_t)2 * its * 9); const auto Ma = io.add<uint64_t>((size_t)2 * its * words);
        const auto W = io.add<uint8_t>(orbm_two_view_workspace_bytes(1, cap_k, its));
        stage_.ensure(R.offset);
        put(stage_, Pb, &P, 1);
        put(stage_, Sets, sets_.data(), sets_.size());
        io_.ensure(io.size());
        check(orb_memcpy_h2d(io_.p, stage_.p, R.offset, stream_), "orb_memcpy_h2d");
        check(orbm_two_view_reconstruct(at(io_, Pb), d_keys1, d_keys2, cap_k, d_matches12, at(io_, Sets), its, 1, at(io_, S), at(io_, Mo), at(io_, Ma),
                                        at(io_, R), at(io_, X), at(io_, T), at(io_, W), stream_),
              "orbm_two_view_reconstruct");
        const size_t len = S.offset - R.offset;
        download(back_.ensure(len), at(io_, R), len, stream_);
        check(orb_stream_sync(stream_), "orb_memcpy_d2h");
        result_ = *downloaded(back_, R, R.offset);
        if (!result_.ok) return false;
        p3d_.assign(downloaded(back_, X, R.offset), downloaded(back_, X, R.offset) + (size_t)cap_k * 3);
        tri_.assign(downloaded(back_, T, R.offset), downloaded(back_, T, R.offset) + cap_k);
        R21.assign(result_.R21, result_.R21 + 9);
        t21.assign(result_.t21, result_.t21 + 3);
        return true;
    }

    float mSigma, fx_ = 0, fy_ = 0, cx_ = 0, cy_ = 0;
    int mMaxIterations;
    void* stream_;
    bool seed_;
    std::vector<int32_t> sets_;
    std::vector<float> p3d_;
    std::vector<uint8_t> tri_;
    orbm_tvr_result result_{};
    detail::DevBuf io_, keys_;
    detail::HostBuf stage_, stage_in_, back_;
};

}  // namespace orbslam3_hip
#endif
