"""Times the device Sim3Solver (orbhip.sim3) on the GPU: problems of N correspondences (60 % outliers) and 300 hypotheses each, one problem
and batches of 8 and 64 in one call.  Warm-up, then the median of `--repeats` event-timed launches in one process (the slabs are written
before the window: the time is orbm_sim3_solve's one kernel), and next to it the count of projections the call performs (two per correspondence
and hypothesis) over that time.

    python tools/sim3_timing.py [--repeats 30] [--n 100] [--its 300] [--batches 1,8,64]"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rot(rng, scale):
    w = rng.normal(size=3) * scale
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def problem(rng, n, its, min_inliers, outliers):
    from orbhip.sim3 import CORR_DTYPE, PROBLEM_DTYPE, RAND_MAX, draw_samples, truncated_max_error
    P = np.zeros((), PROBLEM_DTYPE)
    R1, R2, t1, t2 = rot(rng, 0.3), rot(rng, 0.3), rng.normal(size=3), rng.normal(size=3)
    P["Rcw1"], P["tcw1"], P["Rcw2"], P["tcw2"] = R1.reshape(9), t1, R2.reshape(9), t2
    for cam in ("cam1", "cam2"):
        P[cam]["p"] = [458.654, 457.296, 367.215, 248.375, 0, 0, 0, 0]
    P["min_inliers"], P["max_its"], P["n1"] = min_inliers, its, 2 * n
    X1 = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)], 1)
    R12, t12, s12 = rot(rng, 0.15), rng.normal(size=3) * 0.2, rng.uniform(0.8, 1.25)
    X2 = (X1 - t12) @ R12 / s12 + rng.normal(size=(n, 3)) * 0.002
    bad = rng.random(n) < outliers
    X2[bad] = np.stack([rng.uniform(-2, 2, bad.sum()), rng.uniform(-1.5, 1.5, bad.sum()), rng.uniform(3, 9, bad.sum())], 1)
    C = np.zeros(n, CORR_DTYPE)
    C["Xw1"], C["Xw2"] = (X1 - t1) @ R1, (X2 - t2) @ R2
    C["max_err1"] = C["max_err2"] = truncated_max_error(1.44)
    C["index1"] = rng.permutation(2 * n)[:n]
    return P, C, draw_samples(n, its, rng.integers(0, RAND_MAX + 1, 3 * its))


def main():
    import torch
    from orbhip.sim3 import Sim3Solver
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--its", type=int, default=300)
    ap.add_argument("--batches", default="1,8,64")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    for batch in [int(x) for x in a.batches.split(",")]:
        probs = [problem(rng, a.n, a.its, 20, 0.6) for _ in range(batch)]
        S = Sim3Solver(batch, a.n, a.its, 2 * a.n, device="cuda:0")
        S.set_problems(np.array([p for p, _, _ in probs]), [c for _, c, _ in probs], [s for _, _, s in probs])
        times = []
        for it in range(a.repeats + 5):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            S.launch()
            e1.record()
            torch.cuda.synchronize()
            if it >= 5:
                times.append(e0.elapsed_time(e1) * 1e3)
        res = S.to_host()["result"]
        t = float(np.median(times))
        proj = 2 * batch * a.n * a.its
        print(json.dumps(dict(batch=batch, n=a.n, hypotheses=a.its, median_us=round(t, 1), min_us=round(min(times), 1), max_us=round(max(times), 1),
                              per_problem_us=round(t / batch, 2), projections=proj, gproj_per_s=round(proj / (t * 1e-6) / 1e9, 3),
                              converged=int(res["converged"].sum()), mean_iterations=float(res["iterations"].mean()))), flush=True)


if __name__ == "__main__":
    main()
