"""Times Optimizer::LocalBundleAdjustment on the device map (orbslam3_hip::LocalBundleAdjustment: window build -> lba_optimize(5) ->
lba_optimize(10) -> lba_compute_errors -> write-back) against today's path measured in the same run, at the shape of the other map-side
figures: 31 key frames of about 1000 features and 6000 map points (tests/cpp/local_ba_synth.h), the last key frame the current one, every
other one covisible with it; `--fixed 200` adds 200 key frames of 100 features that are not covisible (fixed).

  run        LocalBundleAdjustment::Run on a resident map: every launch, the read of the result words, the download of the lists and the
             synchronisations (wall clock); the map is uploaded afresh before every run, outside the timed region, because the write-back
             folds the map in place;
  build      orbm_lba_window_build alone, by a pair of HIP events on the NULL stream (with --no-events, for a library without a HIP runtime
             behind it: the wall clock around the call and one synchronisation);
  apply      orbm_lba_window_apply alone on the window the solver left, likewise;
  host       the C++ restatement of tests/cpp/local_ba_host.h (built here with g++ -O3, one core): selection and flattening, then the
             outlier pass, erase loop and write-back fed with the same chi2, depth, poses and points;
  transfer   what the host path moves around its loops: the download of the slabs the flatten reads, the upload of the flattened
             problem, the download of the optimised poses, points, chi2 and depth, the upload of the slabs the write-back changes.
  The three solver calls are the same in both paths and are inside `run` only.  build + apply is the figure to hold against host + transfer.

`--warmup` and `--repeats` runs each; median and min-max, one JSON line per figure.  The two paths' lists and maps are compared on every run.

    python tools/local_ba_timing.py [--repeats 30] [--warmup 5] [--keyframes 31] [--features 1000] [--points 6000] [--fixed 0]"""
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
#include "local_ba_synth.h"
using orbslam3_hip::LocalBundleAdjustment;
namespace detail = orbslam3_hip::detail;
typedef std::chrono::steady_clock Clock;
static double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
static void sync() { detail::check(orb_stream_sync(nullptr), "sync"); }
static void report(const char* what, std::vector<double> v) {
    std::sort(v.begin(), v.end());
    std::printf("{\"what\": \"%s\", \"median_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f, \"runs\": %zu}\n", what, v[v.size() / 2], v.front(), v.back(), v.size());
}
template <class T> static void pull(std::vector<T>& h, const T* d, size_t n) { h.resize(n); if (n) detail::download(h.data(), d, n * sizeof(T), nullptr); }
using lba_synth::DeviceMap;
#ifdef LBA_TIMING_EVENTS
#include <hip/hip_runtime_api.h>
struct Events {   // a pair of events on the NULL stream around one entry point
    hipEvent_t a, b;
    Events() { if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { std::printf("hipEventCreate failed\n"); std::exit(1); } }
    void begin() { (void)hipEventRecord(a, nullptr); }
    double end() { (void)hipEventRecord(b, nullptr); (void)hipEventSynchronize(b); float t = 0; (void)hipEventElapsedTime(&t, a, b); return (double)t; }
};
#define LBA_TIMING_HOW "events"
#else
#define LBA_TIMING_HOW "call + synchronisation"
struct Events {   // the emulated library has no events: the wall clock around the call and one synchronisation
    Clock::time_point t;
    void begin() { t = Clock::now(); }
    double end() { sync(); return ms(t, Clock::now()); }
};
#endif
int main(int argc, char** argv) {
    const int repeats = std::atoi(argv[1]), warmup = std::atoi(argv[2]), n_kf = std::atoi(argv[3]), n_feat = std::atoi(argv[4]), n_mp = std::atoi(argv[5]);
    const int n_fixed = std::atoi(argv[6]);
    (void)argc;
    const lba_synth::World W0 = lba_synth::make(7, n_kf, n_feat, n_mp, n_fixed);
    const lba_host::Map& M0 = W0.M;
    const int cap_p = n_kf + n_fixed + 1, cap_l = n_mp, cap_e = (int)M0.obs.size() + 1;
    LocalBundleAdjustment L;
    L.Configure(W0.cam, cap_p, cap_l, cap_e);
    DeviceMap D;
    detail::DevBuf work, er, wb, res, up[16];
    std::vector<double> t_run, t_build, t_apply, t_host, t_xfer;
    LocalBundleAdjustment::Result R;
    Events ev;
    size_t n_points = 0, n_edges = 0, n_erased = 0, n_bad = 0;
    for (int it = 0; it < warmup + repeats; it++) {
        // ---- the device path
        D.upload(W0); sync();
        auto t0 = Clock::now();
        L.Run(D.V, D.I, D.A, W0.current, W0.init_id, nullptr, R);
        auto t1 = Clock::now();
        if (!R.applied || R.buildFlags || (R.applyFlags & ~ORBM_LBA_EARLY_RETURN)) { std::printf("the device path did not apply (flags %u %u)\n", R.buildFlags, R.applyFlags); return 1; }
        // what the solver left, for the host path and for apply alone
        const orbm_lba_window& w = L.deviceWindow();
        std::vector<double> poses, points, chi2, depth;
        pull(poses, (const double*)w.poses, (size_t)(R.nLocal + R.nFixed) * 7); pull(points, (const double*)w.points, (size_t)R.nPoints * 3);
        pull(chi2, L.deviceChi2(), (size_t)R.nEdges); pull(depth, L.deviceDepth(), (size_t)R.nEdges);
        sync();
        // ---- apply alone, on a fresh map with the window as the solver left it
        D.upload(W0);
        void* wk = work.ensure(orbm_lba_workspace_bytes(D.V.n_kf, D.V.n_mp, D.V.n_obs, D.V.n_kf_mp_rows, D.I.cap_conn, cap_p, cap_l, cap_e) + 16);
        orbm_lba_apply A = D.A;
        A.d_erased = (int32_t*)er.ensure((size_t)cap_e * 8 + 16); A.d_went_bad = (int32_t*)wb.ensure((size_t)cap_l * 4 + 16); A.d_result = (int32_t*)res.ensure(64);
        sync();
        ev.begin();
        detail::check(orbm_lba_window_apply(&D.V, &D.I, &w, L.deviceChi2(), L.deviceDepth(), &A, wk, nullptr), "apply");
        const double ms_apply = ev.end();
        // ---- build alone (it overwrites the window: last)
        D.upload(W0); sync();
        ev.begin();
        detail::check(orbm_lba_window_build(&D.V, &D.I, W0.current, W0.init_id, &w, wk, nullptr), "build");
        const double ms_build = ev.end();
        // ---- the host path: transfers ...
        lba_host::Map H = M0;
        auto x0 = Clock::now();
        pull(H.mp, D.V.d_mp, M0.mp.size()); pull(H.obs_start, D.V.d_obs_start, M0.obs_start.size()); pull(H.obs, D.V.d_obs, M0.obs.size());
        pull(H.kf, D.V.d_kf, M0.kf.size()); pull(H.kf_mp, D.V.d_kf_mp, M0.kf_mp.size()); pull(H.ckf, D.I.d_ckf, M0.ckf.size());
        pull(H.pose, D.I.d_pose, M0.pose.size()); pull(H.kps, D.I.d_kps, M0.kps.size()); pull(H.u_right, D.I.d_u_right, M0.u_right.size());
        pull(H.ordered_kf, D.I.d_ordered_kf, M0.ordered_kf.size()); pull(H.n_ordered, D.I.d_n_ordered, M0.n_ordered.size());
        pull(H.center, (const orbm_keyframe_center*)D.A.d_center, M0.center.size()); pull(H.ref, (const orbm_refresh_point*)D.A.d_ref, M0.ref.size());
        pull(H.nobs, (const int32_t*)D.A.d_mp_nobs, M0.nobs.size());
        sync();
        auto x1 = Clock::now();
        // ... the first host loop
        auto h0 = Clock::now();
        lba_host::Window B = lba_host::build(H, W0.current, W0.init_id, W0.nlevels, W0.inv_sigma2);
        auto h1 = Clock::now();
        auto x2 = Clock::now();
        up[0].upload(B.poses.data(), B.poses.size()); up[1].upload(B.hidx.data(), B.hidx.size()); up[2].upload(B.points.data(), B.points.size());
        up[3].upload(B.edges.data(), B.edges.size()); up[4].upload(B.lm_start.data(), B.lm_start.size()); up[5].upload(B.pose_start.data(), B.pose_start.size());
        up[6].upload(B.pose_edges.data(), B.pose_edges.size());
        sync();
        // (the solver runs here in both paths) ... then its results come back
        std::vector<double> hp, hx, hc, hd;
        pull(hp, (const double*)up[0].p, B.poses.size()); pull(hx, (const double*)up[2].p, B.points.size());
        pull(hc, L.deviceChi2(), B.edges.size()); pull(hd, L.deviceDepth(), B.edges.size());
        sync();
        auto x3 = Clock::now();
        if (B.edges.size() != chi2.size() || B.poses.size() != poses.size()) { std::printf("MISMATCH: the windows differ\n"); return 1; }
        B.poses = poses; B.points = points;
        auto h2 = Clock::now();
        const lba_host::Applied HA = lba_host::apply(H, B, chi2.data(), depth.data(), W0.sf, W0.nlevels);
        auto h3 = Clock::now();
        auto x4 = Clock::now();
        up[7].upload(H.mp.data(), H.mp.size()); up[8].upload(H.kf_mp.data(), H.kf_mp.size()); up[9].upload(H.pose.data(), H.pose.size());
        up[10].upload(H.center.data(), H.center.size()); up[11].upload(H.ref.data(), H.ref.size()); up[12].upload(H.nobs.data(), H.nobs.size());
        up[13].upload(H.obs_start.data(), H.obs_start.size()); up[14].upload(H.obs.data(), H.obs.size());
        sync();
        auto x5 = Clock::now();
        if (HA.erased != R.erased || HA.went_bad != R.wentBad || (int)H.obs.size() != R.nObservationsOut) { std::printf("MISMATCH: the two paths disagree\n"); return 1; }
        n_points = B.point_mp.size(); n_edges = B.edges.size(); n_erased = HA.erased.size(); n_bad = HA.went_bad.size();
        if (it >= warmup) {
            t_run.push_back(ms(t0, t1)); t_apply.push_back(ms_apply); t_build.push_back(ms_build);
            t_host.push_back(ms(h0, h1) + ms(h2, h3)); t_xfer.push_back(ms(x0, x1) + ms(x2, x3) + ms(x4, x5));
        }
    }
    std::printf("{\"what\": \"shape\", \"key_frames\": %zu, \"feature_rows\": %zu, \"map_points\": %zu, \"records\": %zu, \"local\": %d, \"fixed\": %d, \"points\": %zu, \"edges\": %zu, \"erased\": %zu, \"went_bad\": %zu, \"iterations\": [%d, %d]}\n",
                M0.kf.size(), M0.kf_mp.size(), M0.mp.size(), M0.obs.size(), R.nLocal, R.nFixed, n_points, n_edges, n_erased, n_bad, R.iterations[0], R.iterations[1]);
    report("device: LocalBundleAdjustment::Run on a resident map (with the three solver calls)", t_run);
    report("device: orbm_lba_window_build alone (" LBA_TIMING_HOW ")", t_build);
    report("device: orbm_lba_window_apply alone (" LBA_TIMING_HOW ")", t_apply);
    report("host: C++ restatement of selection, flattening and write-back, one core", t_host);
    report("transfer: download of the flatten's inputs, upload of the problem, download of the solver's results, upload of the changed slabs", t_xfer);
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
    ap.add_argument("--fixed", type=int, default=0, help="key frames that are not covisible with the current one (100 features each)")
    ap.add_argument("--lib", default=os.path.join(PKG, "liborbhip.so"))
    ap.add_argument("--no-events", action="store_true", help="time build and apply by the wall clock (the emulated library has no HIP runtime)")
    ap.add_argument("--keep", default=None, help="build the driver to this path and keep it (then run it as: <path> repeats warmup keyframes features points fixed)")
    a = ap.parse_args()
    if a.repeats < 1:
        sys.exit("--repeats must be at least 1")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "lba_timing.cpp"), a.keep or os.path.join(tmp, "lba_timing")
        open(src, "w").write(DRIVER)
        libdir, libname = os.path.dirname(os.path.abspath(a.lib)), os.path.basename(a.lib)[3:-3]
        events = [] if a.no_events else ["-DLBA_TIMING_EVENTS", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
        subprocess.check_call(["g++", "-std=c++17", "-O3", "-ffp-contract=off", "-w"] + events + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"), src,
                               "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"] +
                              ([] if a.no_events else ["-lamdhip64"]) + ["-o", exe])
        if a.keep:
            return
        sys.exit(subprocess.call([exe] + [str(x) for x in (a.repeats, a.warmup, a.keyframes, a.features, a.points, a.fixed)]))


if __name__ == "__main__":
    main()
