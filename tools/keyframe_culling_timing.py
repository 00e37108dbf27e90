"""Times orbm_cull_keyframes and orbm_apply_keyframe_culling on the GPU: 100 candidate key frames of 1000 features over about 6000 map points.

  device   orbm_cull_keyframes for one problem and for a batch of 64 problems on one view (event-timed), then orbm_apply_keyframe_culling;
  host     the C++ restatement of the reference loop (tests/cpp/keyframe_culling_host.h, built here with g++ -O3) on the same flattened input
           (wall clock), one problem after the other;
  upload   the copy of that flattened input from pinned memory to the device, which a caller whose map is not resident would pay first.

5 warm-up and `--repeats` timed runs each; median and min-max, one JSON line per figure.  The two paths' exit codes and events are compared.
--variants name=path,... times further builds of csrc/orbm_culling.hip (e.g. other workgroup sizes, -DCULL_WG=N) for one problem.

    python tools/keyframe_culling_timing.py [--repeats 30] [--batches 1,64] [--variants 64=exp_so/libcull_wg64.so,...]"""
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

HOST = r"""
#include <cstring>
#include "keyframe_culling_host.h"
extern "C" int host_cull(const orbm_map_point* mp, int n_mp, const int32_t* obs_start, const orbm_observation* obs, int n_obs,
                         const orbm_localmap_keyframe* kf, int n_kf, const int32_t* kf_mp, int n_rows, const orbm_cull_keyframe* ckf,
                         const uint8_t* feat, const orbm_cull_problem* P, const int32_t* cands, int n_cands, uint8_t* code, orbm_cull_event* events) {
    static cull_host::Result R;
    cull_host::Map M;
    M.mp = mp; M.n_mp = n_mp; M.obs_start = obs_start; M.obs = obs; M.n_obs = n_obs; M.kf = kf; M.n_kf = n_kf; M.kf_mp = kf_mp;
    M.n_kf_mp_rows = n_rows; M.ckf = ckf; M.feat = feat;
    cull_host::cull(M, *P, cands, n_cands, R);
    std::memcpy(code, R.code.data(), R.code.size());
    std::memcpy(events, R.events.data(), R.events.size() * sizeof(orbm_cull_event));
    return (int)R.events.size();
}
"""


def build_host(tmp):
    src, so = os.path.join(tmp, "host_cull.cpp"), os.path.join(tmp, "host_cull.so")
    open(src, "w").write(HOST)
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           src, "-o", so])
    lib = ctypes.CDLL(so)
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.host_cull.restype = i
    lib.host_cull.argtypes = [vp, i, vp, vp, i, vp, i, vp, i, vp, vp, vp, vp, i, vp, vp]
    return lib


def make_map(rng, n_kf, n_mp, n_feat, max_octave):
    """every key frame has n_feat features, 70 % of them with a point drawn from the whole map, octaves uniform in [0, max_octave);
    observations agree (the first feature that holds a point is the entry's index), in a random pointer order"""
    from orbhip._abi import (CULL_FEAT_CLOSE, CULL_KEYFRAME_DTYPE, LM_KF_PRESENT, LOCALMAP_KEYFRAME_DTYPE, MAP_POINT_DTYPE, MP_HAS_OBS, MP_VALID,
                             OBSERVATION_DTYPE)
    order = rng.permutation(n_kf)
    kf_mp = rng.integers(0, n_mp, (n_kf, n_feat)).astype(np.int32)
    kf_mp[rng.random((n_kf, n_feat)) < 0.3] = -1
    kf = np.zeros(n_kf, LOCALMAP_KEYFRAME_DTYPE)
    kf["flags"], kf["parent"], kf["prev"], kf["covis"] = LM_KF_PRESENT, -1, np.arange(n_kf) - 1, -1
    kf["mp_row0"], kf["n_feat"] = np.arange(n_kf) * n_feat, n_feat
    ckf = np.zeros(n_kf, CULL_KEYFRAME_DTYPE)
    ckf["id"], ckf["prev"], ckf["next"] = np.arange(n_kf), np.arange(n_kf) - 1, np.arange(n_kf) + 1
    ckf["next"][-1] = -1
    ckf["timestamp"], ckf["desc_row0"] = 0.3 * np.arange(n_kf), kf["mp_row0"]
    ckf["imu_pos"] = rng.normal(0, 1, (n_kf, 3))
    feat = (rng.integers(0, max_octave, n_kf * n_feat) | CULL_FEAT_CLOSE).astype(np.uint8)
    seen = [[] for _ in range(n_mp)]
    for k in order:
        pts, first = np.unique(kf_mp[k], return_index=True)
        for p, i in zip(pts, first):
            if p >= 0:
                seen[p].append((k, k * n_feat + i))
    obs_start = np.zeros(n_mp + 1, np.int32)
    obs_start[1:] = np.cumsum([len(s) for s in seen])
    obs = np.zeros(int(obs_start[-1]), OBSERVATION_DTYPE)
    obs["kf"], obs["desc_row"] = [k for s in seen for k, _ in s], [r for s in seen for _, r in s]
    mp = np.zeros(n_mp, MAP_POINT_DTYPE)
    mp["flags"] = MP_VALID | MP_HAS_OBS
    return dict(mp=mp, obs_start=obs_start, obs=obs, kf=kf, kf_mp=kf_mp.reshape(-1)), dict(ckf=ckf, feat=feat, mp_nobs=None)


def stats(name, times, **extra):
    print(json.dumps(dict(what=name, median_us=round(float(np.median(times)), 1), min_us=round(min(times), 1), max_us=round(max(times), 1), **extra)),
          flush=True)


def main():
    import torch
    import orbhip
    from orbhip import _abi, _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--candidates", type=int, default=100)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--octaves", type=int, default=4)
    ap.add_argument("--inertial", action="store_true")
    ap.add_argument("--variants", default="")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    n_kf = a.candidates + 1
    view, cull = make_map(rng, n_kf, a.points, a.features, a.octaves)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (-1,)) if x.dtype.names else np.ascontiguousarray(x)).cuda()  # noqa: E731
    fl = (_abi.CULL_INERTIAL | _abi.CULL_IMU_INITIALIZED) if a.inertial else 0
    libs = [("product", orbhip.ORBmatcher(0.6, False))]
    cull_protos = {k: v for k, v in _abi.PROTOTYPES.items() if "cull" in k}
    for spec in filter(None, a.variants.split(",")):
        name, path = spec.split("=")
        libs.append((name, orbhip.ORBmatcher(0.6, False, lib=_lib.bind(ctypes.CDLL(os.path.join(ROOT, path)), cull_protos))))
    with tempfile.TemporaryDirectory() as tmp:
        H = build_host(tmp)
        for B in [int(x) for x in a.batches.split(",")]:
            pr = np.zeros(B, _abi.CULL_PROBLEM_DTYPE)
            cands = np.concatenate([rng.permutation(a.candidates) for _ in range(B)]).astype(np.int32)
            pr["current_kf"], pr["init_kf_id"], pr["n_cand"], pr["n_kf_in_map"], pr["flags"] = a.candidates, 0xFFFFFFF0, a.candidates, n_kf, fl
            pr["cand_start"] = np.arange(B) * a.candidates
            dv = {k: dev(v) for k, v in view.items()}
            dc = dict(ckf=dev(cull["ckf"]), feat=dev(cull["feat"]), mp_nobs=None)
            d_pr, d_c = dev(pr), dev(cands)
            ref = np.zeros(a.points, _abi.REFRESH_POINT_DTYPE)
            ref["ref_kf"] = view["obs"]["kf"][np.minimum(view["obs_start"][:-1], len(view["obs"]) - 1)]
            results = {}
            for name, m in (libs if B == 1 else libs[:1]):
                out, times = None, []
                for it in range(a.repeats + 5):
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = m.CullKeyFrames(dv, dc, d_pr, d_c, a.candidates, out=out)
                    e1.record()
                    torch.cuda.synchronize()
                    if it >= 5:
                        times.append(e0.elapsed_time(e1) * 1e3)
                m.check_cull_flags(out)
                code, nev = out["code"].cpu().numpy(), out["n_events"].cpu().numpy()
                results[name] = (code, out["events"].cpu().numpy(), nev)
                stats("device_cull", times, build=name, batch=B, candidates=a.candidates, features=a.features, records=int(len(view["obs"])),
                      culled_per_problem=round(float(nev.mean()), 1), per_problem_us=round(float(np.median(times)) / B, 2),
                      workspace_bytes=int(out["work"].numel()))
                if name == "product":
                    times, app = [], None
                    for it in range(a.repeats + 5):   # the apply changes the map: every run starts from a fresh copy of the slabs it writes
                        wv = dict(dv, mp=dev(view["mp"]), kf=dev(view["kf"]), kf_mp=dev(view["kf_mp"]))
                        wc = dict(dc, ckf=dev(cull["ckf"]))
                        d_ref = dev(ref)
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        app = m.ApplyKeyFrameCulling(wv, wc, out, d_ref, len(view["obs"]), problem=0, out=app)
                        e1.record()
                        torch.cuda.synchronize()
                        if it >= 5:
                            times.append(e0.elapsed_time(e1) * 1e3)
                    m.check_cull_applied(app)
                    stats("device_apply", times, batch=B, records_left=int(app["result"].cpu().numpy()[0]))
            # the host restatement, one problem after the other
            h_code = np.zeros((B, a.candidates), np.uint8)
            h_ev = np.zeros((B, a.candidates), _abi.CULL_EVENT_DTYPE)
            h_nev = np.zeros(B, np.int64)
            A = {k: (v.ctypes.data, len(v)) for k, v in list(view.items()) + [("ckf", cull["ckf"]), ("feat", cull["feat"])]}
            times = []
            for it in range(min(a.repeats, 10) + 2):
                t0 = time.perf_counter()
                for b in range(B):
                    h_nev[b] = H.host_cull(A["mp"][0], a.points, A["obs_start"][0], A["obs"][0], A["obs"][1], A["kf"][0], n_kf, A["kf_mp"][0],
                                           A["kf_mp"][1], A["ckf"][0], A["feat"][0], pr[b:b + 1].ctypes.data, cands.ctypes.data, len(cands),
                                           h_code[b].ctypes.data, h_ev[b].ctypes.data)
                if it >= 2:
                    times.append((time.perf_counter() - t0) * 1e6)
            stats("host_restatement", times, batch=B, per_problem_us=round(float(np.median(times)) / B, 2))
            # the upload of the flattened input from pinned memory
            host = [torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).pin_memory()
                    for v in list(view.values()) + [cull["ckf"], cull["feat"]]]
            devs = [torch.empty_like(h, device="cuda") for h in host]
            times = []
            for it in range(a.repeats + 5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for h, d in zip(host, devs):
                    d.copy_(h, non_blocking=True)
                torch.cuda.synchronize()
                if it >= 5:
                    times.append((time.perf_counter() - t0) * 1e6)
            stats("upload_of_the_input", times, bytes=int(sum(h.numel() for h in host)))
            for name, (code, ev, nev) in results.items():
                same = np.array_equal(code, h_code) and np.array_equal(nev, h_nev) and \
                    all(np.array_equal(ev[b, :nev[b]].reshape(-1), h_ev[b, :nev[b]].view(np.uint8).reshape(-1)) for b in range(B))
                if not same:
                    print(json.dumps(dict(error="device and host disagree", build=name, batch=B)), flush=True)
                    sys.exit(1)


if __name__ == "__main__":
    main()
