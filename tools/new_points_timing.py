"""Times the new-map-point kernels on the GPU: 1000 features per key frame, about 300 matches per pair.

  create   orbm_create_new_map_points alone for batches of 1, 20 and 256 pairs in one launch;
  chain    20 neighbours of one current key frame on one stream, search -> create per neighbour, nothing read back in between;
  today    the path a caller has without it, on the same box in the same run: per neighbour the same search, a device-to-host copy of
           match12, the triangulation loop on the host (tests/cpp/new_map_points_host.h, built here with g++ -O3 -ffp-contract=off) and a
           host-to-device copy of the current key frame's has_mp flags.

5 warm-up and `--repeats` timed runs each; create is event-timed, the two chains are wall-clock timed around a final synchronisation (the host
loop is part of one of them).  Median and min-max, one JSON line per figure.

    python tools/new_points_timing.py [--repeats 30] [--batches 1,20,256] [--neighbours 20]"""
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

HOST_LOOP = r"""
#include "new_map_points_host.h"
extern "C" int host_create_loop(const orbm_newpt_pair* P, const orb_keypoint* k1, const orb_keypoint* k2, const int32_t* m12, int n1, uint8_t* h1, uint8_t* h2,
                                orbm_new_point* out, int cap) {
    static std::vector<orbm_new_point> v;
    v.clear();
    const newpt_host::Side S1{k1, nullptr, nullptr, nullptr}, S2{k2, nullptr, nullptr, nullptr};
    const int n = newpt_host::create_loop(*P, S1, S2, m12, n1, h1, h2, v);
    for (int i = 0; i < n && i < cap; i++) out[i] = v[i];
    return n;
}
"""


def build_host_loop(tmp):
    src, so = os.path.join(tmp, "host_loop.cpp"), os.path.join(tmp, "host_loop.so")
    open(src, "w").write(HOST_LOOP)
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.host_create_loop.restype = ctypes.c_int
    lib.host_create_loop.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int]
    return lib


def key_frames(rng, n_feat, n_match, n_neigh):
    """one current key frame and n_neigh neighbours seeing the same planted points; descriptors of corresponding features a few bits apart,
    a synthetic feature vector that keeps them in one node; n_match of the current key frame's features have no map point yet"""
    from orbhip import KP_DTYPE
    from orbhip.matcher import newpt_camera, newpt_pair
    cam = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
    sf = np.cumprod([1.0] + [1.2] * 7).astype(np.float32)
    z = rng.uniform(2, 10, n_feat)
    X = np.stack([rng.uniform(-0.6, 0.6, n_feat) * z, rng.uniform(-0.4, 0.4, n_feat) * z, z], 1)
    base = rng.integers(0, 256, (n_feat, 32), dtype=np.uint8)

    def frame(O, order, has_mp, off_by=None):
        Pc = X - O
        k = np.zeros(n_feat, KP_DTYPE)
        k["x"][order] = cam[0] * Pc[:, 0] / Pc[:, 2] + cam[2]
        k["y"][order] = cam[1] * Pc[:, 1] / Pc[:, 2] + cam[3] + (0 if off_by is None else off_by)
        k["octave"][order] = np.arange(n_feat) % 4
        d = base.copy()
        d[np.arange(n_feat), rng.integers(8, 32, n_feat)] ^= np.uint8(1) << rng.integers(0, 8, n_feat).astype(np.uint8)
        desc = np.zeros_like(d)
        desc[order] = d
        node = desc[:, 0] >> 2
        ids = np.unique(node)
        feat = np.concatenate([np.nonzero(node == i)[0] for i in ids]).astype(np.int32)
        start = np.concatenate([[0], np.cumsum([(node == i).sum() for i in ids])]).astype(np.int32)
        c = newpt_camera(np.eye(3), -O, O, cam, 0.11, 47.9, sf * sf, sf)
        return dict(kps=k, desc=desc, has_mp=has_mp.astype(np.uint8), node_id=ids.astype(np.int32), node_start=start, feat_idx=feat, cam=c)
    has1 = np.ones(n_feat, bool)
    has1[rng.permutation(n_feat)[:n_match]] = False
    kf1 = frame(np.zeros(3), np.arange(n_feat), has1)
    neigh = []
    for i in range(n_neigh):
        a = rng.uniform(0, 2 * np.pi)
        # every neighbour matches all the free features by descriptor, but only its own share of them lies where the geometry says (the others
        # are 30 px off and end at the reprojection gate): about n_match matches per pair for every neighbour of the chain
        off = np.where(np.arange(n_feat) % n_neigh == i, 0.0, 30.0)
        kf2 = frame(np.array([np.cos(a), np.sin(a), 0.0]) * rng.uniform(0.3, 1.0), rng.permutation(n_feat), np.zeros(n_feat, bool), off)
        kf2["pair"] = newpt_pair(kf1["cam"], kf2["cam"], 1.2, kf1=0, kf2=i + 1)
        neigh.append(kf2)
    return kf1, neigh, sf


def side_dev(frames, cap_nodes=64):
    """[B, cap] device arrays of a list of frames, for both wrappers"""
    import torch
    B, n = len(frames), len(frames[0]["kps"])
    o = dict(kps=np.stack([f["kps"] for f in frames]).view(np.float32).reshape(B, n, 7), desc=np.stack([f["desc"] for f in frames]),
             has_mp=np.stack([f["has_mp"] for f in frames]), feat_idx=np.stack([f["feat_idx"] for f in frames]),
             node_id=np.zeros((B, cap_nodes), np.int32), node_start=np.zeros((B, cap_nodes + 1), np.int32),
             n_nodes=np.array([len(f["node_id"]) for f in frames], np.int32), n=np.full(B, n, np.int32))
    for b, f in enumerate(frames):
        o["node_id"][b, :len(f["node_id"])] = f["node_id"]
        o["node_start"][b, :len(f["node_start"])] = f["node_start"]
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in o.items()}


def stats(name, times, **extra):
    print(json.dumps(dict(what=name, median_us=round(float(np.median(times)), 1), min_us=round(min(times), 1), max_us=round(max(times), 1), **extra)),
          flush=True)


def main():
    import torch
    import orbhip
    from orbhip.matcher import NEW_POINT_DTYPE, NEWPT_PAIR_DTYPE, TRI_PAIR_DTYPE
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--batches", default="1,20,256")
    ap.add_argument("--neighbours", type=int, default=20)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=300)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    m = orbhip.ORBmatcher(0.6, False)
    kf1, neigh, sf = key_frames(rng, a.features, a.matches, max(a.neighbours, 1))
    n = a.features
    tri = np.zeros((), TRI_PAIR_DTYPE)
    tri["ep"] = -1e4
    tri["level_sigma2_2"][:8], tri["scale_factors_2"][:8] = sf * sf, sf

    # ---- create alone: `batch` pairs in one launch (the matches come from one search launch before the window)
    for batch in [int(x) for x in a.batches.split(",")]:
        nb = [neigh[b % len(neigh)] for b in range(batch)]
        d1, d2 = side_dev([kf1] * batch), side_dev(nb)
        pairs = torch.from_numpy(np.array([f["pair"] for f in nb], NEWPT_PAIR_DTYPE).view(np.uint8).reshape(batch, -1)).cuda()
        tris = torch.from_numpy(np.array([tri] * batch).view(np.uint8).reshape(batch, -1)).cuda()
        m12, nm = m.SearchForTriangulation(d1, d2, tris, False, True)
        has0 = d1["has_mp"].clone(), d2["has_mp"].clone()
        out, times = None, []
        for it in range(a.repeats + 5):
            d1["has_mp"].copy_(has0[0])
            d2["has_mp"].copy_(has0[1])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = m.CreateNewMapPoints(d1, d2, pairs, m12, n, out=out)
            e1.record()
            torch.cuda.synchronize()
            if it >= 5:
                times.append(e0.elapsed_time(e1) * 1e3)
        stats("create", times, batch=batch, features=n, matches_per_pair=round(float(nm.float().mean()), 1),
              created_per_pair=round(float(out["nnew"].float().mean()), 1), per_pair_us=round(float(np.median(times)) / batch, 2))

    # ---- the neighbour chains
    K = a.neighbours
    d1 = side_dev([kf1])
    d2s = [side_dev([f]) for f in neigh[:K]]
    pairs = [torch.from_numpy(np.array([f["pair"]]).view(np.uint8).reshape(1, -1)).cuda() for f in neigh[:K]]
    tris = torch.from_numpy(np.array([tri]).view(np.uint8).reshape(1, -1)).cuda()
    has0 = d1["has_mp"].clone()
    outs = [None] * K
    times, created = [], 0
    for it in range(a.repeats + 5):
        d1["has_mp"].copy_(has0)
        for d2 in d2s:
            d2["has_mp"].zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(K):
            m12, _ = m.SearchForTriangulation(d1, d2s[k], tris, False, True)
            outs[k] = m.CreateNewMapPoints(d1, d2s[k], pairs[k], m12, n, out=outs[k])
        torch.cuda.synchronize()
        if it >= 5:
            times.append((time.perf_counter() - t0) * 1e6)
    created = int(sum(int(o["nnew"][0]) for o in outs))
    matched = int(sum(int((o["status"] != 0).sum()) for o in outs))
    stats("chain_device", times, neighbours=K, features=n, matches=matched, created=created)

    with tempfile.TemporaryDirectory() as tmp:
        H = build_host_loop(tmp)
        k1 = np.ascontiguousarray(kf1["kps"])
        k2s = [np.ascontiguousarray(f["kps"]) for f in neigh[:K]]
        ps = [np.array([f["pair"]], NEWPT_PAIR_DTYPE) for f in neigh[:K]]
        new = np.zeros(n, NEW_POINT_DTYPE)
        times, created_host = [], 0
        for it in range(a.repeats + 5):
            d1["has_mp"].copy_(has0)
            for d2 in d2s:
                d2["has_mp"].zero_()
            has1 = kf1["has_mp"].copy()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            created_host = 0
            for k in range(K):
                m12, _ = m.SearchForTriangulation(d1, d2s[k], tris, False, True)
                m12_h = m12.cpu().numpy()                                   # D2H of match12 (synchronises)
                has2 = np.zeros(n, np.uint8)
                created_host += H.host_create_loop(ps[k].ctypes.data, k1.ctypes.data, k2s[k].ctypes.data, m12_h.ctypes.data, n, has1.ctypes.data,
                                                   has2.ctypes.data, new.ctypes.data, n)
                d1["has_mp"].copy_(torch.from_numpy(has1).reshape(1, n))    # H2D of the changed flags before the next neighbour's search
            torch.cuda.synchronize()
            if it >= 5:
                times.append((time.perf_counter() - t0) * 1e6)
        stats("chain_today_host_loop", times, neighbours=K, features=n, created=created_host)
    if created != created_host:
        print(json.dumps(dict(error="the two chains created different numbers of points", device=created, host=created_host)), flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
