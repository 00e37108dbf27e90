"""Times LocalMapping::SearchInNeighbors on the device map against the C++ restatement on one host core: a current key frame of 1000
features, 30 targets of 1000 features, about 6000 map points (tests/cpp/search_in_neighbors_synth.h).

  device     orbslam3_hip::SearchInNeighbors::Run on a resident map: every launch of orbm_search_in_neighbors, the download of the results and
             the synchronisation (wall clock); the map is uploaded afresh before every run, outside the timed region, because the call folds
             the map in place;
  host       the restatement of tests/cpp/search_in_neighbors_host.h (built here with g++ -O3) on a fresh copy of the same flattened map (wall
             clock, the copy outside the timed region);
  transfer   the upload of the flattened map plus the download of the slabs a host fuse changes: what a caller whose map lives on the
             device pays around a host fuse today.  host + transfer is the figure to hold against device.

`--warmup` and `--repeats` runs each; median and min-max, one JSON line per figure.  The two paths' events are compared on every run.

    python tools/search_in_neighbors_timing.py [--repeats 30] [--warmup 5] [--keyframes 31] [--features 1000] [--true-points 4000] [--see 0.5]"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "awesome-orb-slam3-3dvisioncraft-version_amd")

DRIVER = r"""
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "orbslam3_hip/LocalMapping.h"
#include "search_in_neighbors_synth.h"
using orbslam3_hip::SearchInNeighbors;
typedef std::chrono::steady_clock Clock;
static double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
static void report(const char* what, std::vector<double> v, size_t events) {
    std::sort(v.begin(), v.end());
    std::printf("{\"what\": \"%s\", \"median_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f, \"runs\": %zu, \"events\": %zu}\n", what, v[v.size() / 2],
                v.front(), v.back(), v.size(), events);
}
int main(int argc, char** argv) {
    const int repeats = std::atoi(argv[1]), warmup = std::atoi(argv[2]), n_kf = std::atoi(argv[3]), n_feat = std::atoi(argv[4]), n_true = std::atoi(argv[5]);
    const double see = std::atof(argv[6]);
    (void)argc;
    const fusenb_synth::World W0 = fusenb_synth::make(7, n_kf, n_true, see, n_feat);
    SearchInNeighbors::Camera C;
    C.fx = W0.P.fx; C.fy = W0.P.fy; C.cx = W0.P.cx; C.cy = W0.P.cy; C.mbf = W0.P.mbf; C.th = W0.P.th;
    for (int i = 0; i < 4; i++) C.bounds[i] = W0.P.bounds[i];
    C.grid = W0.P.grid;
    C.scaleFactors.assign(W0.P.scale_factors, W0.P.scale_factors + 8);
    C.invLevelSigma2.assign(W0.P.inv_level_sigma2, W0.P.inv_level_sigma2 + 8);
    C.logScaleFactor = W0.lsf;
    SearchInNeighbors S;
    S.SetCamera(C);
    SearchInNeighbors::Settings T;
    T.capTargets = 40; T.capCandidates = (int)W0.M.mp.size() + 1; T.capEvents = 4 * n_feat + (int)W0.M.mp.size();
    T.capObservations = (int)(W0.M.obs.size() + W0.M.kf_mp.size());
    std::printf("{\"what\": \"shape\", \"key_frames\": %d, \"features_current\": %d, \"map_points\": %zu, \"records\": %zu, \"feature_rows\": %zu}\n", n_kf,
                W0.M.kf[W0.current].n_feat, W0.M.mp.size(), W0.M.obs.size(), W0.M.kf_mp.size());
    std::vector<double> dev, host, xfer;
    size_t events = 0;
    for (int it = 0; it < warmup + repeats; it++) {
        fusenb_synth::World W = W0;
        fusenb_host::Map& M = W.M;
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
        V.maxFeatures = W.max_feat;
        auto t0 = Clock::now();
        S.SetMap(V);
        auto t1 = Clock::now();
        SearchInNeighbors::Result D;
        const bool abort = false;
        auto t2 = Clock::now();
        S.Run(W.current, T, &abort, D);
        auto t3 = Clock::now();
        // what a host fuse would have to bring back and send again: the slabs the fusion changes
        const orbm_fusenb_out& O = S.deviceOutputs();
        std::vector<uint8_t> sink(std::max({M.mp.size() * sizeof(orbm_map_point), M.kf_mp.size() * 4, M.mp_desc.size(), M.obs.size() * sizeof(orbm_observation)}));
        auto t4 = Clock::now();
        orbslam3_hip::detail::download(sink.data(), O.d_mp, M.mp.size() * sizeof(orbm_map_point), nullptr);
        orbslam3_hip::detail::download(sink.data(), O.d_kf_mp, M.kf_mp.size() * 4, nullptr);
        orbslam3_hip::detail::download(sink.data(), O.d_mp_desc, M.mp_desc.size(), nullptr);
        orbslam3_hip::detail::download(sink.data(), S.deviceMap().d_obs, M.obs.size() * sizeof(orbm_observation), nullptr);
        orbslam3_hip::detail::check(orb_stream_sync(nullptr), "sync");
        auto t5 = Clock::now();
        orbm_fusenb_params P = W.P;
        P.current_kf = W.current; P.flags = 0;
        fusenb_host::Result H;
        auto t6 = Clock::now();
        fusenb_host::Fuser(M, P, W.lsf, T.capTargets, T.capCandidates, T.capEvents).run(H);
        auto t7 = Clock::now();
        if (D.events.size() != H.events.size() || D.targets != H.targets || D.replaced != H.replaced) { std::printf("MISMATCH\n"); return 1; }
        for (size_t i = 0; i < H.events.size(); i++)
            if (D.events[i].point != H.events[i].point || D.events[i].feature != H.events[i].feature || D.events[i].kind != H.events[i].kind) { std::printf("MISMATCH\n"); return 1; }
        events = H.events.size();
        if (it >= warmup) { dev.push_back(ms(t2, t3)); host.push_back(ms(t6, t7)); xfer.push_back(ms(t0, t1) + ms(t4, t5)); }
    }
    report("device: SearchInNeighbors::Run on a resident map", dev, events);
    report("host: C++ restatement, one core", host, events);
    report("transfer: map upload + download of the changed slabs", xfer, events);
    return 0;
}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=31)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--true-points", type=int, default=4000)
    ap.add_argument("--see", type=float, default=0.5, help="the chance that a key frame sees a true point in its image: with the defaults about 6000 map points")
    ap.add_argument("--lib", default=os.path.join(PKG, "liborbhip.so"))
    a = ap.parse_args()
    if a.repeats < 1:
        sys.exit("--repeats must be at least 1")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "sin_timing.cpp"), os.path.join(tmp, "sin_timing")
        open(src, "w").write(DRIVER)
        libdir, libname = os.path.dirname(os.path.abspath(a.lib)), os.path.basename(a.lib)[3:-3]
        subprocess.check_call(["g++", "-std=c++17", "-O3", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"), src, "-L", libdir,
                               "-l" + libname, "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
        sys.exit(subprocess.call([exe] + [str(x) for x in (a.repeats, a.warmup, a.keyframes, a.features, a.true_points, a.see)]))


if __name__ == "__main__":
    main()
