// orbslam3_hip/Sim3Solver.h — adapter for ORB_SLAM3::Sim3Solver (reference include/Sim3Solver.h, src/Sim3Solver.cc) over liborbhip.so
// (include/orbhip.h "Sim3Solver"): the RANSAC Horn alignment LoopClosing::DetectCommonRegionsFromBoW runs between SearchByBoW(KF, KF) and the
// Sim3 projection search (LoopClosing.cc:640-830).
//
// The reference's constructor gathers its correspondences from KeyFrame / MapPoint objects (:35-124); this class takes them flattened
// (orbm_sim3_problem + orbm_sim3_corr, the gather loop is shown in INTEGRATION.md "Sim3Solver") and carries the reference's member
// signatures from there on.  A cv::Mat result is a std::vector<float> here: 16 floats, the row-major 4x4 mT12i; empty where the reference
// returns cv::Mat().
//
// How it differs from the reference, and why the answers do not:
//  * The FIRST iterate() / find() evaluates every hypothesis of the problem in one launch (orbm_sim3_solve) and downloads their inlier counts,
//    masks and transforms.  That and every later call then walk the reference's loop (:170-218, :243-296) over those numbers, so any chunking
//    (`iterate(20)` in a loop, LoopClosing.cc:754-757; find()) returns what the reference returns, including the calls after a convergence
//    (mnBestInliers persists) and after bNoMore.
//  * All mRansacMaxIts triples are therefore drawn UP FRONT, with rand() through DUtils::Random::RandomInt's formula and the swap-with-back
//    removal (:175-189).  The triples are the ones the reference's lazy draws would produce from the same rand() state, but the global rand()
//    stream advances by 3 * mRansacMaxIts at the first call even when the solver converges early: code that shares rand() with the solver
//    sees different numbers afterwards than next to the reference.
//  * SetRansacParameters after the first iterate() discards the evaluated hypotheses; the next iterate() draws and launches again.
#ifndef ORBSLAM3_HIP_SIM3SOLVER_H
#define ORBSLAM3_HIP_SIM3SOLVER_H
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "detail/DeviceIO.h"

namespace orbslam3_hip {

class Sim3Solver {
public:
    // problem: Rcw1 / tcw1 / Rcw2 / tcw2, the two cameras and n1 = vpMatched12.size() (fix_scale, min_inliers and max_its are set here and by
    // SetRansacParameters); corr: the correspondences that survive the constructor's filters, in its order.
    Sim3Solver(const orbm_sim3_problem& problem, const std::vector<orbm_sim3_corr>& corr, const bool bFixScale, void* stream = nullptr)
        : prob_(problem), corr_(corr), stream_(stream) {
        prob_.fix_scale = bFixScale ? 1 : 0;
        mN1 = prob_.n1;
        N = (int)corr_.size();
        if (N > ORBM_SIM3_MAX_N) throw std::invalid_argument("Sim3Solver: more than ORBM_SIM3_MAX_N correspondences");
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        if (minInliers < 3) throw std::invalid_argument("Sim3Solver: minInliers below 3");   // a Horn alignment needs three pairs
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        mRansacMaxIts = orbm_sim3_ransac_iterations(probability, minInliers, maxIterations, N);
        mnIterations = 0;
        launched_ = false;
    }

    std::vector<float> iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        bool bConverge;
        std::vector<float> T = iterate(nIterations, bNoMore, vbInliers, nInliers, bConverge);
        return bConverge ? T : std::vector<float>();   // the first overload returns cv::Mat() unless it converged (:218)
    }

    std::vector<float> iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge) {
        bNoMore = false;
        bConverge = false;
        vbInliers.assign((size_t)(mN1 > 0 ? mN1 : 0), false);
        nInliers = 0;
        if (N < mRansacMinInliers) {
            bNoMore = true;
            return std::vector<float>();
        }
        if (!launched_) Launch();
        int nCurrentIterations = 0;
        std::vector<float> bestSim3;
        while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
            nCurrentIterations++;
            const int h = mnIterations++;
            if (count_[h] >= mnBestInliers) {
                mnBestInliers = count_[h];
                best_ = hyp_[h];   // mBestRotation / mBestTranslation / mBestScale are clones: they outlive a relaunch
                hasBest_ = true;
                if (count_[h] > mRansacMinInliers) {
                    nInliers = count_[h];
                    for (int i = 0; i < N; i++)
                        if (Inlier(h, i) && corr_[i].index1 >= 0 && corr_[i].index1 < mN1) vbInliers[corr_[i].index1] = true;
                    bConverge = true;
                    return T12(h);
                }
                bestSim3 = T12(h);
            }
        }
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return bestSim3;
    }

    std::vector<float> find(std::vector<bool>& vbInliers12, int& nInliers) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }

    // mBestRotation (9 floats, row-major), mBestTranslation (3), mBestScale; empty / 0 before any hypothesis became the best
    std::vector<float> GetEstimatedRotation() const { return hasBest_ ? std::vector<float>(best_.R12, best_.R12 + 9) : std::vector<float>(); }
    std::vector<float> GetEstimatedTranslation() const { return hasBest_ ? std::vector<float>(best_.t12, best_.t12 + 3) : std::vector<float>(); }
    float GetEstimatedScale() const { return hasBest_ ? best_.s12 : 0.f; }

    // what the launch produced (valid after the first iterate() of a problem with N >= minInliers)
    int MaxIterations() const { return mRansacMaxIts; }
    int Iterations() const { return mnIterations; }
    int BestInliers() const { return mnBestInliers; }
    const std::vector<int32_t>& HypothesisCounts() const { return count_; }
    const std::vector<orbm_sim3_hyp>& Hypotheses() const { return hyp_; }
    const std::vector<int32_t>& Samples() const { return samples_; }   // [MaxIterations()][3]
    const orbm_sim3_result& DeviceResult() const { return result_; }   // the device's own pick: what find() on a fresh solver returns
    bool Inlier(int h, int i) const { return (mask_[(size_t)h * words_ + (size_t)(i >> 6)] >> (i & 63)) & 1u; }
    std::vector<float> T12(int h) const {   // mT12i: sR = ms12i*mR12i (each element times the double scale, rounded once), mt12i
        std::vector<float> T(16, 0.f);
        const orbm_sim3_hyp& H = hyp_[h];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) T[i * 4 + j] = (float)((double)H.R12[i * 3 + j] * (double)H.s12);
            T[i * 4 + 3] = H.t12[i];
        }
        T[15] = 1.f;
        return T;
    }

    // DUtils::Random::RandomInt(min, max) (Thirdparty/DBoW2/DUtils/Random.cpp:47-50)
    static int RandomInt(int min, int max) {
        const int d = max - min + 1;
        return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
    }

private:
    void Launch() {
        const int its = mRansacMaxIts;
        samples_.assign((size_t)its * 3, 0);
        std::vector<int32_t> avail;
        for (int h = 0; h < its; h++) {   // :175-189
            avail.resize(N);
            for (int i = 0; i < N; i++) avail[i] = i;   // vAvailableIndices = mvAllIndices
            for (int i = 0; i < 3; i++) {
                const int randi = RandomInt(0, (int)avail.size() - 1);
                samples_[(size_t)h * 3 + i] = avail[randi];
                avail[randi] = avail.back();
                avail.pop_back();
            }
        }
        prob_.min_inliers = mRansacMinInliers;
        prob_.max_its = its;
        words_ = (N + 63) / 64;
        const int capN1 = mN1 > 0 ? mN1 : 1;
        // one device block: [problem | corr | n | samples || hyp | count | mask | result || inliers | work]; upload [0, H), download [H, I)
        using namespace detail;
        Layout io;
        const auto P = io.add<orbm_sim3_problem>(1); const auto C = io.add<orbm_sim3_corr>(N); const auto Nn = io.add<int32_t>(1);
        const auto S = io.add<int32_t>((size_t)its * 3); const auto H = io.add<orbm_sim3_hyp>(its); const auto Cnt = io.add<int32_t>(its);
        const auto M = io.add<uint64_t>((size_t)its * words_); const auto R = io.add<orbm_sim3_result>(1); const auto I = io.add<uint8_t>(capN1);
        const auto W = io.add<uint8_t>(orbm_sim3_workspace_bytes(1, N, its));
        stage_.ensure(H.offset);
        put(stage_, P, &prob_, 1);
        put(stage_, C, corr_.data(), N);
        put(stage_, Nn, &N, 1);
        put(stage_, S, samples_.data(), samples_.size());
        io_.ensure(io.size());
        check(orb_memcpy_h2d(io_.p, stage_.p, H.offset, stream_), "orb_memcpy_h2d");
        check(orbm_sim3_solve(at(io_, P), at(io_, C), at(io_, Nn), N, at(io_, S), its, 1, at(io_, H), at(io_, Cnt), at(io_, M), at(io_, R), at(io_, I), capN1,
                              at(io_, W), stream_),
              "orbm_sim3_solve");
        const size_t len = I.offset - H.offset;
        download(back_.ensure(len), at(io_, H), len, stream_);
        check(orb_stream_sync(stream_), "orb_memcpy_d2h");
        hyp_.assign(downloaded(back_, H, H.offset), downloaded(back_, H, H.offset) + its);
        count_.assign(downloaded(back_, Cnt, H.offset), downloaded(back_, Cnt, H.offset) + its);
        mask_.assign(downloaded(back_, M, H.offset), downloaded(back_, M, H.offset) + (size_t)its * words_);
        result_ = *downloaded(back_, R, H.offset);
        launched_ = true;
    }

    orbm_sim3_problem prob_;
    std::vector<orbm_sim3_corr> corr_;
    void* stream_;
    int N = 0, mN1 = 0, mnIterations = 0, mnBestInliers = 0, mRansacMinInliers = 6, mRansacMaxIts = 300, words_ = 0;
    double mRansacProb = 0.99;
    bool launched_ = false, hasBest_ = false;
    orbm_sim3_hyp best_{};
    std::vector<int32_t> samples_, count_;
    std::vector<uint64_t> mask_;
    std::vector<orbm_sim3_hyp> hyp_;
    orbm_sim3_result result_{};
    detail::DevBuf io_;
    detail::HostBuf stage_, back_;
};

}  // namespace orbslam3_hip
#endif
