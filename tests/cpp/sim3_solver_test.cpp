// sim3_solver_test.cpp — the control flow of the header-only adapter orbslam3_hip::Sim3Solver: chunked iterate() (chunks of 1, 20 and
// mRansacMaxIts), both overloads, find(), a continuation call after a convergence and one after bNoMore, against a plain serial replay of the
// reference's loops (Sim3Solver.cc:152-297) that runs on the adapter's own downloaded per-hypothesis counts.  Only control flow is under test
// here; the numbers are the business of tests/test_sim3_solver.py.  Built with g++ against the emulated library (CPU tier) and liborbhip.so
// (GPU tier).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include <orbslam3_hip/Sim3Solver.h>

namespace {
int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); fails++; } } while (0)

double urand(unsigned& s) { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / 16777216.0; }

// a scene: camera-1 points, camera-2 points = the inverse of a known Sim3 applied to them, the first nOut replaced by random points
void make_scene(int n, int nOut, unsigned seed, orbm_sim3_problem& P, std::vector<orbm_sim3_corr>& C) {
    std::memset(&P, 0, sizeof(P));
    for (int i = 0; i < 3; i++) P.Rcw1[i * 4] = P.Rcw2[i * 4] = 1.f;
    for (orbm_sim3_camera* cam : {&P.cam1, &P.cam2}) { cam->model = ORBM_SIM3_CAM_PINHOLE; cam->p[0] = 458.f; cam->p[1] = 457.f; cam->p[2] = 367.f; cam->p[3] = 248.f; }
    P.n1 = n + 5;
    const double a = 0.2, s = 1.1, t[3] = {0.1, -0.05, 0.2};   // X1 = s Rz(a) X2 + t
    C.assign(n, orbm_sim3_corr{});
    for (int i = 0; i < n; i++) {
        const double x = -2 + 4 * urand(seed), y = -1.5 + 3 * urand(seed), z = 3 + 6 * urand(seed);
        double q[3] = {(x - t[0]) / s, (y - t[1]) / s, (z - t[2]) / s};
        double x2 = std::cos(a) * q[0] + std::sin(a) * q[1], y2 = -std::sin(a) * q[0] + std::cos(a) * q[1], z2 = q[2];
        if (i < nOut) { x2 = -2 + 4 * urand(seed); y2 = -1.5 + 3 * urand(seed); z2 = 3 + 6 * urand(seed); }
        C[i].Xw1[0] = (float)x; C[i].Xw1[1] = (float)y; C[i].Xw1[2] = (float)z;
        C[i].Xw2[0] = (float)x2; C[i].Xw2[1] = (float)y2; C[i].Xw2[2] = (float)z2;
        C[i].max_err1 = C[i].max_err2 = 13.f;   // (size_t)(9.210 * 1.44)
        C[i].index1 = (i * 11) % P.n1;           // distinct: 11 and n1 are coprime in the scenes below
    }
}

// the reference's members and loops, on given per-hypothesis counts
struct Replay {
    const std::vector<int32_t>& count;
    int N, minInliers, maxIts, mnIterations = 0, mnBestInliers = 0, best = -1;
    // -> the hypothesis whose T12 is returned (-1: cv::Mat()); `second` selects the overload with bConverge
    int iterate(int nIterations, bool second, bool& bNoMore, int& nInliers, bool& bConverge, int& inlierHyp) {
        bNoMore = false; bConverge = false; nInliers = 0; inlierHyp = -1;
        if (N < minInliers) { bNoMore = true; return -1; }
        int nCurrentIterations = 0, bestSim3 = -1;
        while (mnIterations < maxIts && nCurrentIterations < nIterations) {
            nCurrentIterations++;
            const int h = mnIterations++;
            if (count[h] >= mnBestInliers) {
                mnBestInliers = count[h];
                best = h;
                if (count[h] > minInliers) { nInliers = count[h]; inlierHyp = h; bConverge = true; return h; }
                else if (second) bestSim3 = h;
            }
        }
        if (mnIterations >= maxIts) bNoMore = true;
        return bestSim3;
    }
};

// drives the adapter and the replay side by side: chunks until convergence or bNoMore (LoopClosing.cc:754-757), then `extra` continuation calls
void drive(const char* what, int n, int nOut, int minInliers, int maxIts, int chunk, bool second, int extra, bool wantConverge) {
    orbm_sim3_problem P;
    std::vector<orbm_sim3_corr> C;
    make_scene(n, nOut, 99u, P, C);
    orbslam3_hip::Sim3Solver S(P, C, false);
    S.SetRansacParameters(0.99, minInliers, maxIts);
    if (chunk <= 0) chunk = S.MaxIterations();
    std::srand(5);   // the adapter draws at its first iterate()
    std::vector<int32_t> noCounts;
    Replay* R = nullptr;
    bool everConverged = false, everNoMore = false;
    int calls = 0, extraLeft = extra;
    for (;;) {
        bool bNoMore = false, bConverge = false;
        std::vector<bool> vbInliers;
        int nInliers = -1;
        const std::vector<float> T = second ? S.iterate(chunk, bNoMore, vbInliers, nInliers, bConverge) : S.iterate(chunk, bNoMore, vbInliers, nInliers);
        if (!R) R = new Replay{n >= minInliers ? S.HypothesisCounts() : noCounts, n, minInliers, S.MaxIterations()};   // the counts exist after the first call
        bool rNoMore, rConverge;
        int rInliers, rInlierHyp;
        const int rh = R->iterate(chunk, second, rNoMore, rInliers, rConverge, rInlierHyp);
        calls++;
        CHECK(bNoMore == rNoMore && nInliers == rInliers && (!second || bConverge == rConverge), "%s call %d: noMore %d/%d inliers %d/%d converge %d/%d", what,
              calls, bNoMore, rNoMore, nInliers, rInliers, bConverge, rConverge);
        CHECK(S.Iterations() == R->mnIterations && S.BestInliers() == R->mnBestInliers, "%s call %d: mnIterations %d/%d mnBestInliers %d/%d", what, calls,
              S.Iterations(), R->mnIterations, S.BestInliers(), R->mnBestInliers);
        if (rh < 0) CHECK(T.empty(), "%s call %d: a transform where the reference returns cv::Mat()", what, calls);
        else CHECK(T == S.T12(rh) && T.size() == 16 && T[15] == 1.f, "%s call %d: not the transform of hypothesis %d", what, calls, rh);
        CHECK((int)vbInliers.size() == P.n1, "%s: vbInliers has %d entries", what, (int)vbInliers.size());
        std::vector<bool> want(P.n1, false);
        if (rInlierHyp >= 0)
            for (int i = 0; i < n; i++) if (S.Inlier(rInlierHyp, i)) want[C[i].index1] = true;
        int trues = 0;
        for (bool v : vbInliers) trues += v;
        CHECK(vbInliers == want && trues == rInliers, "%s call %d: vbInliers (%d set, %d inliers)", what, calls, trues, rInliers);
        if (R->best >= 0) {
            const orbm_sim3_hyp& H = S.Hypotheses()[R->best];
            const std::vector<float> Rm = S.GetEstimatedRotation(), tm = S.GetEstimatedTranslation();
            const float sm = S.GetEstimatedScale();
            CHECK(Rm.size() == 9 && tm.size() == 3 && !std::memcmp(Rm.data(), H.R12, 36) && !std::memcmp(tm.data(), H.t12, 12) && !std::memcmp(&H.s12, &sm, 4), "%s call %d: GetEstimated* are not hypothesis %d", what, calls, R->best);
        }
        const bool done = rNoMore || rConverge || (!second && rh >= 0);
        everConverged |= rh >= 0 && rInlierHyp >= 0;
        everNoMore |= rNoMore;
        if (done && extraLeft-- <= 0) break;
        if (calls > 4 * maxIts + 8) { CHECK(false, "%s: does not end", what); break; }
    }
    CHECK(everConverged == wantConverge, "%s: converged %d, the scene was built for %d", what, everConverged, wantConverge);
    if (!wantConverge) CHECK(everNoMore, "%s: bNoMore was never set", what);
    if (n >= minInliers) {
        // the triples: drawn up front with rand(), distinct and in range; the device's own pick = the replay of find() on a fresh solver
        const std::vector<int32_t>& sm = S.Samples();
        CHECK((int)sm.size() == 3 * S.MaxIterations(), "%s: %d sample entries", what, (int)sm.size());
        std::srand(5);
        bool same = true, distinct = true;
        std::vector<int32_t> avail;
        for (int h = 0; h < S.MaxIterations(); h++) {
            avail.resize(n);
            for (int i = 0; i < n; i++) avail[i] = i;
            for (int i = 0; i < 3; i++) {
                const int randi = int(((double)std::rand() / ((double)RAND_MAX + 1.0)) * (int)avail.size());
                same &= sm[h * 3 + i] == avail[randi];
                avail[randi] = avail.back();
                avail.pop_back();
            }
            distinct &= std::set<int32_t>(sm.begin() + h * 3, sm.begin() + h * 3 + 3).size() == 3;
        }
        CHECK(same && distinct, "%s: the triples are not RandomInt's on rand() after srand(5)", what);
        Replay F{S.HypothesisCounts(), n, minInliers, S.MaxIterations()};
        bool fNoMore, fConverge;
        int fInliers, fHyp;
        F.iterate(S.MaxIterations(), true, fNoMore, fInliers, fConverge, fHyp);
        const orbm_sim3_result& D = S.DeviceResult();
        CHECK(D.iterations == F.mnIterations && D.converged == (int)fConverge && D.no_more == (int)fNoMore && D.best_iter == F.best &&
              D.n_inliers == F.mnBestInliers && D.status == 0u, "%s: device pick %d %d %d %d %d, replay %d %d %d %d %d", what, D.iterations, D.converged,
              D.no_more, D.best_iter, D.n_inliers, F.mnIterations, fConverge, fNoMore, F.best, F.mnBestInliers);
    }
    delete R;
}
}  // namespace

int main() {
    // 60 correspondences, 36 outliers: converges after a few iterations; min_inliers 20 of 24 inliers
    for (int chunk : {1, 20, 0}) {
        drive("converging, first overload", 60, 36, 20, 120, chunk, false, 1, true);
        drive("converging, second overload", 60, 36, 20, 120, chunk, true, 2, true);
    }
    // 30 correspondences, 22 outliers, min_inliers 12: never converges, runs into bNoMore; then one more call
    for (int chunk : {1, 20, 0}) {
        drive("never converging, first overload", 30, 22, 12, 45, chunk, false, 1, false);
        drive("never converging, second overload", 30, 22, 12, 45, chunk, true, 1, false);
    }
    // fewer correspondences than min_inliers: bNoMore at once, nothing launched
    drive("too few", 5, 0, 6, 50, 20, true, 1, false);
    {   // find() = iterate(mRansacMaxIts) of the first overload; SetRansacParameters' clamp; minInliers < 3 is refused
        orbm_sim3_problem P;
        std::vector<orbm_sim3_corr> C;
        make_scene(60, 36, 99u, P, C);
        orbslam3_hip::Sim3Solver S(P, C, true);
        S.SetRansacParameters(0.99, 20, 300);
        CHECK(S.MaxIterations() == orbm_sim3_ransac_iterations(0.99, 20, 300, 60) && S.MaxIterations() > 100 && S.MaxIterations() < 150, "MaxIterations %d", S.MaxIterations());
        std::srand(5);
        std::vector<bool> in;
        int nIn = 0;
        const std::vector<float> T = S.find(in, nIn);
        const orbm_sim3_result& D = S.DeviceResult();
        CHECK(D.converged == (int)!T.empty() && nIn == (D.converged ? D.n_inliers : 0) && S.Iterations() == D.iterations, "find: %d %d %d", (int)T.empty(), nIn, D.iterations);
        if (!T.empty()) CHECK(!std::memcmp(T.data(), D.T12, 64) && S.GetEstimatedScale() == 1.f, "find: T12 differs from the device's result record");
        bool threw = false;
        try { S.SetRansacParameters(0.99, 2, 300); } catch (const std::invalid_argument&) { threw = true; }
        CHECK(threw, "minInliers 2 was accepted");
    }
    if (fails) { std::printf("sim3_solver_test: %d failure(s)\n", fails); return 1; }
    std::printf("sim3_solver_test OK\n");
    return 0;
}
