"""Times orbm_update_connections and orbm_erase_connections on the GPU: 101 key frames of 1000 features over 6000 map points (about 66 k records).

  device   orbm_update_connections for a list of one key frame (ProcessNewKeyFrame) and of 100 (the loop of CorrectLoop), and
           orbm_erase_connections for 22 cull events on the graph the 101 updates leave (event-timed; every run starts from the same store);
  host     the C++ restatement (tests/cpp/covisibility_host.h, built here with g++ -O3) on the same flattened input (wall clock);
  upload   the copy of that flattened input from pinned memory to the device, which a caller whose map is not resident would pay first.

5 warm-up and `--repeats` timed runs each; median and min-max, one JSON line per figure.  The two paths' weight maps and ordered lists are
compared after every case.

    python tools/covisibility_timing.py [--repeats 30]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOST = r"""
#include <chrono>
#include <cstring>
#include "covisibility_host.h"
// updates `list` on an empty graph (after `n_before` untimed updates of the key frames 0 .. n_before-1), then erases `events`; -> microseconds of
// the timed part (the list when n_list > 0, else the erase); the final n_conn / n_ordered / ordered rows go to the out arrays
extern "C" double host_covis(const orbm_map_point* mp, int n_mp, const int32_t* obs_start, const orbm_observation* obs, const orbm_localmap_keyframe* kf,
                             int n_kf, const int32_t* kf_mp, const int32_t* order, const orbm_covis_keyframe* ckf, int n_before, const int32_t* list,
                             int n_list, const int32_t* events, int n_events, int cap, int32_t* n_conn, int32_t* n_ordered, int32_t* okf) {
    covis_host::Map M;
    M.mp = mp; M.n_mp = n_mp; M.obs_start = obs_start; M.obs = obs; M.kf = kf; M.n_kf = n_kf; M.kf_mp = kf_mp; M.kf_by_order = order;
    covis_host::Graph G(M, std::vector<orbm_covis_keyframe>(ckf, ckf + n_kf));
    for (int k = 0; k < n_before; k++) covis_host::update_connections(M, G, k, 0xFFFFFFF0u);
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n_list; i++) covis_host::update_connections(M, G, list[i], 0xFFFFFFF0u);
    const auto t1 = std::chrono::steady_clock::now();
    for (int i = 0; i < n_events; i++) covis_host::erase_connections(G, events[i]);
    const auto t2 = std::chrono::steady_clock::now();
    for (int k = 0; k < n_kf; k++) {
        n_conn[k] = (int32_t)G.conn[k].size(); n_ordered[k] = (int32_t)G.okf[k].size();
        for (size_t j = 0; j < G.okf[k].size() && (int)j < cap; j++) okf[(size_t)k * cap + j] = G.okf[k][j];
    }
    return std::chrono::duration<double, std::micro>(n_list > 0 ? t1 - t0 : t2 - t1).count();
}
"""


def build_host(tmp):
    src, so = os.path.join(tmp, "host_covis.cpp"), os.path.join(tmp, "host_covis.so")
    open(src, "w").write(HOST)
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           src, "-o", so])
    lib = ctypes.CDLL(so)
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.host_covis.restype = ctypes.c_double
    lib.host_covis.argtypes = [vp, i, vp, vp, vp, i, vp, vp, vp, i, vp, i, vp, i, i, vp, vp, vp]
    return lib


def stats(name, times, **extra):
    print(json.dumps(dict(what=name, median_us=round(float(np.median(times)), 1), min_us=round(min(times), 1), max_us=round(max(times), 1), **extra)),
          flush=True)


def main():
    import torch
    from keyframe_culling_timing import make_map
    from orbhip import _abi
    from orbhip.covisibility import CovisibilityGraph
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--keyframes", type=int, default=101)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--events", type=int, default=22)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    n_kf, cap = a.keyframes, a.keyframes
    view, _ = make_map(rng, n_kf, a.points, a.features, 4)
    view["kf_by_order"] = rng.permutation(n_kf).astype(np.int32)
    ckf = np.zeros(n_kf, _abi.COVIS_KEYFRAME_DTYPE)
    ckf["id"], ckf["flags"] = np.arange(n_kf), _abi.COVIS_KF_FIRST_CONNECTION
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (-1,)) if x.dtype.names else np.ascontiguousarray(x)).cuda()  # noqa: E731
    dv = {k: dev(v) for k, v in view.items()}
    i32 = lambda *sh: torch.zeros(sh, dtype=torch.int32, device="cuda")   # noqa: E731
    store = dict(conn=torch.zeros((n_kf, cap, 8), dtype=torch.uint8, device="cuda"), n_conn=i32(n_kf), ordered_kf=i32(n_kf, cap),
                 ordered_w=i32(n_kf, cap), n_ordered=i32(n_kf))
    d_ckf = dev(ckf)
    G = CovisibilityGraph(store, d_ckf, lib=None)
    kf0, ckf0 = dv["kf"].clone(), d_ckf.clone()

    def reset(saved=None):
        for k, v in store.items():
            v.zero_() if saved is None else v.copy_(saved[k])
        dv["kf"].copy_(kf0 if saved is None else saved["kf"])
        d_ckf.copy_(ckf0 if saved is None else saved["ckf"])

    def timed(call, saved=None):
        out, times = None, []
        for it in range(a.repeats + 5):
            reset(saved)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call(out)
            e1.record()
            torch.cuda.synchronize()
            if it >= 5:
                times.append(e0.elapsed_time(e1) * 1e3)
        G.check_flags(out)
        return times

    with tempfile.TemporaryDirectory() as tmp:
        H = build_host(tmp)
        A = {k: v.ctypes.data for k, v in view.items()}
        h_nc, h_no, h_okf = np.zeros(n_kf, np.int32), np.zeros(n_kf, np.int32), np.zeros((n_kf, cap), np.int32)

        def host(n_before, lst, events):
            lst, events = np.ascontiguousarray(lst, np.int32), np.ascontiguousarray(events, np.int32)   # (a field of a record array is strided)
            times = []
            for it in range(min(a.repeats, 10) + 2):
                t = H.host_covis(A["mp"], a.points, A["obs_start"], A["obs"], A["kf"], n_kf, A["kf_mp"], A["kf_by_order"], ckf.ctypes.data, n_before,
                                 lst.ctypes.data, len(lst), events.ctypes.data, len(events), cap, h_nc.ctypes.data, h_no.ctypes.data, h_okf.ctypes.data)
                if it >= 2:
                    times.append(t)
            return times

        def same():
            nc, no, okf = store["n_conn"].cpu().numpy(), store["n_ordered"].cpu().numpy(), store["ordered_kf"].cpu().numpy()
            if not (np.array_equal(nc, h_nc) and np.array_equal(no, h_no) and all(np.array_equal(okf[k, :no[k]], h_okf[k, :no[k]]) for k in range(n_kf))):
                print(json.dumps(dict(error="device and host disagree")), flush=True)
                sys.exit(1)

        for n_list in (1, n_kf - 1):
            lst = rng.permutation(n_kf)[:n_list].astype(np.int32)
            d_list = dev(lst)
            t = timed(lambda out: G.UpdateConnections(dv, d_list, 0xFFFFFFF0, out=out))
            stats("device_update_connections", t, n_list=n_list, key_frames=n_kf, features=a.features, records=int(len(view["obs"])),
                  per_key_frame_us=round(float(np.median(t)) / n_list, 2), workspace_bytes=int(G.Workspace(n_list).numel()))
            th = host(0, lst, [])
            stats("host_restatement_update", th, n_list=n_list, per_key_frame_us=round(float(np.median(th)) / n_list, 2))
            same()
        # the erase, on the graph that one update of every key frame leaves
        reset()
        G.UpdateConnections(dv, dev(np.arange(n_kf, dtype=np.int32)), 0xFFFFFFF0)
        torch.cuda.synchronize()
        saved = dict({k: v.clone() for k, v in store.items()}, kf=dv["kf"].clone(), ckf=d_ckf.clone())
        ev = np.zeros(a.events, _abi.CULL_EVENT_DTYPE)
        ev["kf"] = rng.permutation(n_kf)[:a.events]
        d_ev, d_n = dev(ev), dev(np.asarray([a.events], np.int32))
        t = timed(lambda out: G.EraseConnections(dv, d_ev, d_n, out=out), saved)
        stats("device_erase_connections", t, events=a.events, key_frames=n_kf)
        th = host(n_kf, [], ev["kf"])
        stats("host_restatement_erase", th, events=a.events)
        same()
        # the upload of the flattened input from pinned memory
        host_arrays = [torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).pin_memory() for v in list(view.values()) + [ckf]]
        devs = [torch.empty_like(h, device="cuda") for h in host_arrays]
        times = []
        for it in range(a.repeats + 5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for h, d in zip(host_arrays, devs):
                d.copy_(h, non_blocking=True)
            torch.cuda.synchronize()
            if it >= 5:
                times.append((time.perf_counter() - t0) * 1e6)
        stats("upload_of_the_input", times, bytes=int(sum(h.numel() for h in host_arrays)))


if __name__ == "__main__":
    main()
