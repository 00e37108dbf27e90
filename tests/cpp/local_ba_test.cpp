// local_ba_test.cpp — the adapter orbslam3_hip::LocalBundleAdjustment (include/orbslam3_hip/Optimizer.h) on a device-resident map against
// the C++ restatement of tests/cpp/local_ba_host.h: the window as built, bytes (poseFromTcw included), at the stop-flag exit before the
// first optimise; the exit between the two optimisations (bDoMore false); the whole chain; the folded map against the restatement fed with
// the call's own chi2, depth, poses and points; a window that does not fit its slabs (std::length_error, the map untouched).
#include <cstdio>
#include <cstdlib>

#include "local_ba_synth.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)
using orbslam3_hip::LocalBundleAdjustment;
namespace detail = orbslam3_hip::detail;

template <class T> static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
using lba_synth::fetch;
using lba_synth::DeviceMap;

static bool same_map(const lba_host::Map& a, const lba_host::Map& b) {
    const bool parts[8] = {same(a.mp, b.mp), same(a.kf_mp, b.kf_mp), same(a.pose, b.pose), same(a.center, b.center), same(a.ref, b.ref),
                           same(a.nobs, b.nobs), same(a.obs_start, b.obs_start), same(a.obs, b.obs)};
    bool all = true;
    for (int i = 0; i < 8; i++) {
        if (!parts[i]) std::printf("the maps differ in part %d (mp, kf_mp, pose, center, ref, nobs, obs_start, obs)\n", i);
        all = all && parts[i];
    }
    return all;
}

// the adapter with the stop flag raised right after the first optimise: LocalMapping raising it while that optimise ran its last trial
struct RaisingAdapter : LocalBundleAdjustment {
    bool* flag = nullptr;
    void afterFirstOptimize() override { if (flag) *flag = true; }
};

// the restatement fed with the call's own numbers -> the map and the lists it leaves
static void check_applied(const lba_synth::World& W0, const lba_host::Window& B, LocalBundleAdjustment& L, const DeviceMap& D,
                          const LocalBundleAdjustment::Result& R) {
    const orbm_lba_window& w = L.deviceWindow();
    lba_host::Window O = B;
    O.poses = fetch((const double*)w.poses, B.poses.size());
    O.points = fetch((const double*)w.points, B.points.size());
    const std::vector<double> chi2 = fetch(L.deviceChi2(), B.edges.size()), depth = fetch(L.deviceDepth(), B.edges.size());
    lba_host::Map H = W0.M;
    const lba_host::Applied A = lba_host::apply(H, O, chi2.data(), depth.data(), W0.sf, W0.nlevels);
    CHECK(A.early == R.earlyReturn && !A.early && R.applied);
    CHECK(A.erased == R.erased && A.went_bad == R.wentBad && !R.erased.empty());
    CHECK((int)H.obs.size() == R.nObservationsOut);
    CHECK(same_map(H, D.download(W0.M, true, R.nObservationsOut)));
    CHECK(!same(H.pose, W0.M.pose) && !same(H.mp, W0.M.mp));   // it really wrote
}

int main() {
    const lba_synth::World W0 = lba_synth::make(5, 8, 60, 300, 2, 30);
    const lba_host::Window B = lba_host::build(W0.M, W0.current, W0.init_id, W0.nlevels, W0.inv_sigma2);
    const int np = (int)B.hidx.size(), nl = (int)B.point_mp.size(), ne = (int)B.edges.size();
    std::printf("window: %d poses, %d points, %d edges, %d fixed, num_fixedKF %d, flags %u\n", np, nl, ne, B.n_fixed, B.num_fixed, B.flags);
    CHECK(B.flags == 0 && np == 10 && nl > 100 && ne > 300 && B.n_fixed == 2 && B.num_fixed == 3);   // (two fixed key frames and the init key frame, which is local)
    RaisingAdapter L;
    L.Configure(W0.cam, np + 2, nl + 3, ne + 5);
    DeviceMap D;
    LocalBundleAdjustment::Result R;
    {   // the stop flag before the first optimise: the window as built, bytes, and the map untouched
        D.upload(W0);
        bool stop = true;
        L.Run(D.V, D.I, D.A, W0.current, W0.init_id, &stop, R);
        CHECK(R.stoppedBeforeOptimize && !R.applied && !R.didMore && R.buildFlags == 0);
        CHECK(R.num_fixedKF == B.num_fixed && R.nLocal == B.n_local && R.nFixed == B.n_fixed && R.nPoints == nl && R.nEdges == ne);
        const orbm_lba_window& w = L.deviceWindow();
        CHECK(same(fetch((const double*)w.poses, (size_t)np * 7), B.poses));   // LbaLinearizer::poseFromTcw, operation for operation
        CHECK(same(fetch((const int32_t*)w.pose_hidx, np), B.hidx) && same(fetch((const double*)w.points, (size_t)nl * 3), B.points));
        CHECK(same(fetch((const lba_edge*)w.edges, ne), B.edges) && same(fetch((const int32_t*)w.d_edge_rec, ne), B.edge_rec));
        CHECK(same(fetch((const int32_t*)w.lm_start, nl + 1), B.lm_start) && same(fetch((const int32_t*)w.pose_start, np + 1), B.pose_start));
        CHECK(same(fetch((const int32_t*)w.pose_edges, ne), B.pose_edges) && same(fetch((const int32_t*)w.d_pose_kf, np), B.pose_kf));
        CHECK(same(fetch((const int32_t*)w.d_pose_local, np), B.pose_local) && same(fetch((const int32_t*)w.d_point_mp, nl), B.point_mp));
        CHECK(same_map(W0.M, D.download(W0.M, false, 0)));
    }
    {   // the flag raised between the two optimisations: bDoMore is false, the outlier pass and the write-back still run
        D.upload(W0);
        bool stop = false;
        L.flag = &stop;
        L.Run(D.V, D.I, D.A, W0.current, W0.init_id, &stop, R);
        L.flag = nullptr;
        CHECK(!R.stoppedBeforeOptimize && !R.didMore && R.iterations[0] >= 1 && R.iterations[1] == 0);
        check_applied(W0, B, L, D, R);
    }
    {   // the whole chain, no stop flag
        D.upload(W0);
        L.Run(D.V, D.I, D.A, W0.current, W0.init_id, nullptr, R);
        CHECK(R.didMore && R.iterations[0] >= 1 && R.iterations[1] >= 1 && R.num_fixedKF == B.num_fixed);
        check_applied(W0, B, L, D, R);
    }
    {   // a window that does not fit its slabs: reported, the map untouched
        LocalBundleAdjustment S;
        S.Configure(W0.cam, np + 2, nl - 1, ne + 5);
        D.upload(W0);
        bool threw = false;
        try { S.Run(D.V, D.I, D.A, W0.current, W0.init_id, nullptr, R); } catch (const std::length_error&) { threw = true; }
        CHECK(threw && same_map(W0.M, D.download(W0.M, false, 0)));
    }
    std::printf("local_ba_test OK\n");
    return 0;
}
