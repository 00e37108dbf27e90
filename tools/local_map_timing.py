"""Times orbm_update_local_map on the GPU: a frame of 1000 features, 100 local key frames of 1000 features, about 6000 local map points.

  device   orbm_update_local_map for batches of 1, 8 and 64 frames in one call (event-timed);
  today    the path a caller has without it, on the same inputs in the same run: the host restatement of UpdateLocalKeyFrames +
           UpdateLocalPoints + the marking loop (tests/cpp/local_map_host.h, built here with g++ -O3) frame by frame, then the copy of the
           records and track entries it produced from pinned memory to the device (wall clock around a final synchronisation).

5 warm-up and `--repeats` timed runs each; median and min-max, one JSON line per figure.  The two paths' point lists are compared.

    python tools/local_map_timing.py [--repeats 30] [--batches 1,8,64]"""
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
#include "local_map_host.h"
extern "C" int host_update_local_map(const orbm_map_point* mp, int n_mp, const int32_t* obs_start, const orbm_observation* obs, int n_obs,
                                     const orbm_localmap_keyframe* kf, int n_kf, const int32_t* kf_mp, int n_rows, const int32_t* children,
                                     int n_children, const int32_t* order, const orbm_track* slab, int last_kf, unsigned flags, int32_t* vote,
                                     int n_vote, orbm_map_point* out_mp, orbm_track* out_trk, int32_t* out_src, int32_t* out_nkf) {
    static localmap_host::Scratch S;
    static localmap_host::Result R;
    localmap_host::Map M;
    M.mp = mp; M.n_mp = n_mp; M.obs_start = obs_start; M.obs = obs; M.n_obs = n_obs; M.kf = kf; M.n_kf = n_kf; M.kf_mp = kf_mp;
    M.n_kf_mp_rows = n_rows; M.children = children; M.n_children = n_children; M.kf_by_order = order;
    const orbm_localmap_frame F{last_kf, flags};
    localmap_host::update(M, F, vote, n_vote, vote, n_vote, nullptr, 0, slab, S, R);
    const size_t n = R.local_src.size();
    std::memcpy(out_mp, R.local_mp.data(), n * sizeof(orbm_map_point));   // into the pinned staging block
    std::memcpy(out_trk, R.track.data(), n * sizeof(orbm_track));
    std::memcpy(out_src, R.local_src.data(), n * 4);
    *out_nkf = (int)R.local_kf.size();
    return (int)n;
}
"""


def build_host(tmp):
    src, so = os.path.join(tmp, "host_local_map.cpp"), os.path.join(tmp, "host_local_map.so")
    open(src, "w").write(HOST)
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           src, "-o", so])
    lib = ctypes.CDLL(so)
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.host_update_local_map.restype = i
    lib.host_update_local_map.argtypes = [vp, i, vp, vp, i, vp, i, vp, i, vp, i, vp, vp, i, ctypes.c_uint, vp, i, vp, vp, vp, vp]
    return lib


def make_map(rng, n_kf, n_mp, n_feat):
    """every key frame sees n_feat features, 70 % of them with a point drawn from the whole map; observations agree, in pointer order"""
    from orbhip._abi import LM_KF_PRESENT, LOCALMAP_KEYFRAME_DTYPE, MAP_POINT_DTYPE, MP_HAS_OBS, MP_VALID, OBSERVATION_DTYPE, TRACK_DTYPE
    order = rng.permutation(n_kf).astype(np.int32)
    rank = np.empty(n_kf, np.int64)
    rank[order] = np.arange(n_kf)
    kf_mp = rng.integers(0, n_mp, (n_kf, n_feat)).astype(np.int32)
    kf_mp[rng.random((n_kf, n_feat)) < 0.3] = -1
    kf = np.zeros(n_kf, LOCALMAP_KEYFRAME_DTYPE)
    kf["flags"], kf["prev"] = LM_KF_PRESENT, np.arange(n_kf) - 1
    kf["parent"] = [-1] + [int(rng.integers(0, k)) for k in range(1, n_kf)]
    kf["mp_row0"], kf["n_feat"] = np.arange(n_kf) * n_feat, n_feat
    kf["covis"] = rng.integers(0, n_kf, (n_kf, 10))
    kids = [sorted(np.nonzero(kf["parent"] == k)[0], key=lambda c: rank[c]) for k in range(n_kf)]
    kf["n_child"] = [len(c) for c in kids]
    kf["child_start"] = np.concatenate([[0], np.cumsum(kf["n_child"])[:-1]])
    children = np.array([c for cs in kids for c in cs], np.int32)
    seen = [[] for _ in range(n_mp)]
    for k in order:   # pointer order
        for p in np.unique(kf_mp[k][kf_mp[k] >= 0]):
            seen[p].append(k)
    obs_start = np.zeros(n_mp + 1, np.int32)
    obs_start[1:] = np.cumsum([len(s) for s in seen])
    obs = np.zeros(int(obs_start[-1]), OBSERVATION_DTYPE)
    obs["kf"] = [k for s in seen for k in s]
    mp = np.zeros(n_mp, MAP_POINT_DTYPE)
    mp["pos"], mp["desc_row"], mp["flags"] = rng.normal(0, 3, (n_mp, 3)), np.arange(n_mp), MP_VALID | MP_HAS_OBS
    track = np.zeros(n_mp, TRACK_DTYPE)
    track["in_view"], track["proj_x"] = rng.integers(0, 2, n_mp), rng.uniform(0, 700, n_mp)
    return dict(mp=mp, obs_start=obs_start, obs=obs, kf=kf, kf_mp=kf_mp.reshape(-1), children=children, kf_by_order=order, mp_track=track)


def stats(name, times, **extra):
    print(json.dumps(dict(what=name, median_us=round(float(np.median(times)), 1), min_us=round(min(times), 1), max_us=round(max(times), 1), **extra)),
          flush=True)


def main():
    import torch
    import orbhip
    from orbhip._abi import LOCALMAP_FRAME_DTYPE, MAP_POINT_DTYPE, TRACK_DTYPE
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--keyframes", type=int, default=100)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--points", type=int, default=6000)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    m = orbhip.ORBmatcher(0.6, False)
    W = make_map(rng, a.keyframes, a.points, a.features)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (-1,)) if x.dtype.names else np.ascontiguousarray(x)).cuda()  # noqa: E731
    nf, n_mp, cap_kf = a.features, a.points, max(a.keyframes, 128)
    with tempfile.TemporaryDirectory() as tmp:
        H = build_host(tmp)
        for B in [int(x) for x in a.batches.split(",")]:
            votes = rng.integers(0, n_mp, (B, nf)).astype(np.int32)
            votes[rng.random((B, nf)) < 0.3] = -1
            view = {k: dev(v) for k, v in W.items()}
            view["mp_track"] = dev(np.repeat(W["mp_track"][None], B, 0)) if B > 1 else view["mp_track"]
            fr = np.zeros(B, LOCALMAP_FRAME_DTYPE)
            fr["last_kf"] = -1
            d_fr, d_vote, d_n = dev(fr), dev(votes), dev(np.full(B, nf, np.int32))
            out, times = None, []
            for it in range(a.repeats + 5):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = m.UpdateLocalMap(view, d_fr, d_vote, d_n, d_vote, d_n, cap_kf, n_mp, out=out)
                e1.record()
                torch.cuda.synchronize()
                if it >= 5:
                    times.append(e0.elapsed_time(e1) * 1e3)
            m.check_local_map(out)
            nkf, nmp = out["n_local_kf"].cpu().numpy(), out["nmp"].cpu().numpy()
            stats("device", times, batch=B, features=nf, local_keyframes=round(float(nkf.mean()), 1), local_points=round(float(nmp.mean()), 1),
                  per_frame_us=round(float(np.median(times)) / B, 2), workspace_bytes=int(out["work"].numel() * 4))
            # today: the host restatement frame by frame, then the records and tracks from pinned memory to the device
            pin_mp = torch.zeros((B, n_mp, MAP_POINT_DTYPE.itemsize), dtype=torch.uint8).pin_memory()
            pin_trk = torch.zeros((B, n_mp, TRACK_DTYPE.itemsize), dtype=torch.uint8).pin_memory()
            d_mp, d_trk = torch.zeros_like(pin_mp, device="cuda"), torch.zeros_like(pin_trk, device="cuda")
            src, nkf_h = np.zeros((B, n_mp), np.int32), np.zeros(1, np.int32)
            A = {k: (v.ctypes.data, len(v)) for k, v in W.items()}
            times, n_host = [], np.zeros(B, np.int64)
            for it in range(a.repeats + 5):
                hv = votes.copy()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for b in range(B):
                    n_host[b] = H.host_update_local_map(A["mp"][0], n_mp, A["obs_start"][0], A["obs"][0], A["obs"][1], A["kf"][0], A["kf"][1],
                                                        A["kf_mp"][0], A["kf_mp"][1], A["children"][0], A["children"][1], A["kf_by_order"][0],
                                                        A["mp_track"][0], -1, 0, hv[b].ctypes.data, nf, pin_mp[b].data_ptr(),
                                                        pin_trk[b].data_ptr(), src[b].ctypes.data, nkf_h.ctypes.data)
                    d_mp[b, :n_host[b]].copy_(pin_mp[b, :n_host[b]], non_blocking=True)
                    d_trk[b, :n_host[b]].copy_(pin_trk[b, :n_host[b]], non_blocking=True)
                torch.cuda.synchronize()
                if it >= 5:
                    times.append((time.perf_counter() - t0) * 1e6)
            stats("today_host_and_upload", times, batch=B, features=nf, local_points=round(float(n_host.mean()), 1),
                  per_frame_us=round(float(np.median(times)) / B, 2), uploaded_bytes=int(n_host.sum()) * 80)
            same = all(np.array_equal(out["local_src"][b, :nmp[b]].cpu().numpy(), src[b, :n_host[b]]) for b in range(B)) and \
                np.array_equal(nmp, n_host) and torch.equal(out["local_mp"][0, :nmp[0]].cpu(), pin_mp[0, :nmp[0]])
            if not same:
                print(json.dumps(dict(error="the two paths built different local maps", batch=B)), flush=True)
                sys.exit(1)


if __name__ == "__main__":
    main()
