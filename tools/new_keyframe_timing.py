"""Times the head of LocalMapping::Run on the device map, ProcessNewKeyFrame's association loop and MapPointCulling, against the C++
restatement on one host core: 31 key frames of about 1000 features, the last one the new key frame, about 6000 map points and a recent list
of 300 (tests/cpp/new_keyframe_synth.h).

  device     orbslam3_hip::ProcessNewKeyFrame::Run then orbslam3_hip::MapPointCulling::Run on a resident map: every launch, the downloads
             of the results and the synchronisations (wall clock); the map is uploaded afresh before every run, outside the timed region,
             because the calls fold the map in place;
  host       the restatement of tests/cpp/new_keyframe_host.h (built here with g++ -O3) on a fresh copy of the same flattened map, both
             steps (wall clock, the copy outside the timed region);
  transfer   the upload of the flattened map plus the download of the slabs the two steps change: what a caller whose map lives on the
             device pays around the two host loops today.  host + transfer is the figure to hold against device.

`--warmup` and `--repeats` runs each; median and min-max, one JSON line per figure.  The two paths' codes are compared on every run.

    python tools/new_keyframe_timing.py [--repeats 30] [--warmup 5] [--keyframes 31] [--features 1000] [--points 6000] [--recent 300]"""
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
#include "new_keyframe_synth.h"
#include "orbslam3_hip/LocalMapping.h"
using orbslam3_hip::MapPointCulling;
using orbslam3_hip::NewKeyFrameMap;
using orbslam3_hip::ProcessNewKeyFrame;
typedef std::chrono::steady_clock Clock;
static double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
static void report(const char* what, std::vector<double> v, size_t added, size_t culled) {
    std::sort(v.begin(), v.end());
    std::printf("{\"what\": \"%s\", \"median_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f, \"runs\": %zu, \"added\": %zu, \"culled\": %zu}\n", what,
                v[v.size() / 2], v.front(), v.back(), v.size(), added, culled);
}
int main(int argc, char** argv) {
    const int repeats = std::atoi(argv[1]), warmup = std::atoi(argv[2]), n_kf = std::atoi(argv[3]), n_feat = std::atoi(argv[4]), n_mp = std::atoi(argv[5]);
    const int n_recent = std::atoi(argv[6]);
    (void)argc;
    const newkf_synth::World W0 = newkf_synth::make(7, n_kf, n_feat, n_mp, n_recent);
    ProcessNewKeyFrame P;
    P.SetScaleFactors(std::vector<float>(W0.sf, W0.sf + W0.nlevels));
    MapPointCulling C;
    std::printf("{\"what\": \"shape\", \"key_frames\": %d, \"features_current\": %d, \"map_points\": %zu, \"records\": %zu, \"feature_rows\": %zu, \"recent\": %zu}\n",
                n_kf, W0.M.kf[W0.current].n_feat, W0.M.mp.size(), W0.M.obs.size(), W0.M.kf_mp.size(), W0.M.recent.size());
    std::vector<double> dev, devP, devC, host, xfer;
    size_t added = 0, culled = 0;
    for (int it = 0; it < warmup + repeats; it++) {
        newkf_synth::World W = W0;
        newkf_host::Map& M = W.M;
        NewKeyFrameMap::MapView V;
        V.map.mapPoints = M.mp.data(); V.map.nMapPoints = (int)M.mp.size(); V.map.obsStart = M.obs_start.data(); V.map.observations = M.obs.data();
        V.map.nObservations = (int)M.obs.size(); V.map.keyFrames = M.kf.data(); V.map.nKeyFrames = (int)M.kf.size();
        V.map.keyFrameMapPoints = M.kf_mp.data(); V.map.nKeyFrameMapPointRows = (int)M.kf_mp.size(); V.map.cullKeyFrames = M.ckf.data();
        V.map.features = M.feat.data(); V.map.mapPointObservations = M.nobs.data();
        V.refPoints = M.ref.data(); V.centers = M.center.data();
        V.keyFrameDescriptors = M.kf_desc.data(); V.nKeyFrameDescriptorRows = (int)(M.kf_desc.size() / 32);
        V.mapPointDescriptors = M.mp_desc.data(); V.nMapPointDescriptorRows = (int)(M.mp_desc.size() / 32);
        V.pointerOrder = M.kf_by_order.data(); V.found = M.found.data(); V.visible = M.visible.data(); V.firstKeyFrameIds = M.first.data();
        V.recent = M.recent; V.maxFeatures = W.max_feat;
        V.capObservations = (int)M.obs.size() + W.max_feat; V.capRecent = n_recent + W.max_feat;
        auto t0 = Clock::now();
        P.SetMap(V);
        auto t1 = Clock::now();
        ProcessNewKeyFrame::Result D;
        MapPointCulling::Result E;
        auto t2 = Clock::now();
        P.Run(W.current, D);
        auto t2b = Clock::now();
        C.UseDeviceMap(P.deviceSlabs());
        C.Run(W.current, false, E);
        auto t3 = Clock::now();
        // what the two host loops would have to bring back and send again: the slabs they change
        const orbslam3_hip::NewKeyFrameSlabs& S = C.deviceSlabs();
        std::vector<uint8_t> sink(std::max({M.mp.size() * sizeof(orbm_map_point), M.kf_mp.size() * 4, M.mp_desc.size(), (size_t)S.view.n_obs * sizeof(orbm_observation)}));
        auto t4 = Clock::now();
        orbslam3_hip::detail::download(sink.data(), S.d_mp, M.mp.size() * sizeof(orbm_map_point), nullptr);
        orbslam3_hip::detail::download(sink.data(), S.d_kf_mp, M.kf_mp.size() * 4, nullptr);
        orbslam3_hip::detail::download(sink.data(), S.d_mp_desc, M.mp_desc.size(), nullptr);
        orbslam3_hip::detail::download(sink.data(), S.view.d_obs, (size_t)S.view.n_obs * sizeof(orbm_observation), nullptr);
        orbslam3_hip::detail::check(orb_stream_sync(nullptr), "sync");
        auto t5 = Clock::now();
        newkf_host::Result H1, H2;
        newkf_host::Mapper K(M, W.sf, W.nlevels);   // (mObservations as the host holds them: not part of the loops)
        auto t6 = Clock::now();
        {
            K.process_new_keyframe(W.current, V.capRecent, V.capObservations, H1);
            K.cull_map_points(W.current, false, V.capObservations, H2);
        }
        auto t7 = Clock::now();
        if (D.added != H1.sel || E.codes != H2.code || E.culled != H2.sel || E.recent != M.recent) { std::printf("MISMATCH\n"); return 1; }
        added = H1.sel.size(); culled = H2.sel.size();
        if (it >= warmup) { dev.push_back(ms(t2, t3)); devP.push_back(ms(t2, t2b)); devC.push_back(ms(t2b, t3)); host.push_back(ms(t6, t7)); xfer.push_back(ms(t0, t1) + ms(t4, t5)); }
    }
    report("device: ProcessNewKeyFrame::Run + MapPointCulling::Run on a resident map", dev, added, culled);
    report("device: ProcessNewKeyFrame::Run alone", devP, added, culled);
    report("device: MapPointCulling::Run alone", devC, added, culled);
    report("host: C++ restatement of both loops, one core", host, added, culled);
    report("transfer: map upload + download of the changed slabs", xfer, added, culled);
    return 0;
}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=31)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--recent", type=int, default=300)
    ap.add_argument("--lib", default=os.path.join(PKG, "liborbhip.so"))
    ap.add_argument("--keep", default=None, help="build the driver to this path and keep it (then run it as: <path> repeats warmup keyframes features points recent)")
    a = ap.parse_args()
    if a.repeats < 1:
        sys.exit("--repeats must be at least 1")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "nk_timing.cpp"), a.keep or os.path.join(tmp, "nk_timing")
        open(src, "w").write(DRIVER)
        libdir, libname = os.path.dirname(os.path.abspath(a.lib)), os.path.basename(a.lib)[3:-3]
        subprocess.check_call(["g++", "-std=c++17", "-O3", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"), src, "-L", libdir,
                               "-l" + libname, "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
        if a.keep:
            return
        sys.exit(subprocess.call([exe] + [str(x) for x in (a.repeats, a.warmup, a.keyframes, a.features, a.points, a.recent)]))


if __name__ == "__main__":
    main()
