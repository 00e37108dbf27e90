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

#include "ORBmatcher.h"

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
        // one device block: [problem | corr | n | samples || hyp | count | mask | result || inliers | work]; upload [0, oH), download [oH, oI)
        size_t off = 0;
        auto sec = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
        const size_t oP = sec(sizeof(orbm_sim3_problem)), oC = sec((size_t)N * sizeof(orbm_sim3_corr)), oN = sec(4), oS = sec((size_t)its * 12),
                     oH = sec((size_t)its * sizeof(orbm_sim3_hyp)), oCnt = sec((size_t)its * 4), oM = sec((size_t)its * words_ * 8),
                     oR = sec(sizeof(orbm_sim3_result)), oI = sec((size_t)capN1), oW = sec(orbm_sim3_workspace_bytes(1, N, its));
        (void)oP;
        uint8_t* stage = stage_.ensure(oH);
        std::memcpy(stage + oP, &prob_, sizeof(prob_));
        std::memcpy(stage + oC, corr_.data(), (size_t)N * sizeof(orbm_sim3_corr));
        const int32_t n = N;
        std::memcpy(stage + oN, &n, 4);
        std::memcpy(stage + oS, samples_.data(), (size_t)its * 12);
        uint8_t* d = (uint8_t*)io_.ensure(off);
        if (orb_memcpy_h2d(d, stage, oH, stream_) != ORB_OK) throw std::runtime_error("orb_memcpy_h2d");
        if (orbm_sim3_solve((const orbm_sim3_problem*)(d + oP), (const orbm_sim3_corr*)(d + oC), (const int32_t*)(d + oN), N, (const int32_t*)(d + oS), its,
                            1, (orbm_sim3_hyp*)(d + oH), (int32_t*)(d + oCnt), (uint64_t*)(d + oM), (orbm_sim3_result*)(d + oR), d + oI, capN1, d + oW,
                            stream_) != ORB_OK)
            throw std::runtime_error("orbm_sim3_solve");
        uint8_t* back = back_.ensure(oI - oH);
        if (orb_memcpy_d2h(back, d + oH, oI - oH, stream_) != ORB_OK || orb_stream_sync(stream_) != ORB_OK) throw std::runtime_error("orb_memcpy_d2h");
        hyp_.resize(its);
        count_.resize(its);
        mask_.resize((size_t)its * words_);
        std::memcpy(hyp_.data(), back, (size_t)its * sizeof(orbm_sim3_hyp));
        std::memcpy(count_.data(), back + (oCnt - oH), (size_t)its * 4);
        std::memcpy(mask_.data(), back + (oM - oH), (size_t)its * words_ * 8);
        std::memcpy(&result_, back + (oR - oH), sizeof(result_));
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
