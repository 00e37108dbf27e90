"""Times the device TwoViewReconstruction (orbhip.two_view) on the GPU: frame pairs with N matches out of n keys (20 % wrong matches, 0.1 px
noise) and 200 iterations each, one problem and batches of 8 and 64 in one call.  5 warm-up calls, then `--repeats` event-timed calls in one
process (the slabs are written before the window: the time is orbm_two_view_reconstruct's four kernels); median and min-max.

    python tools/two_view_timing.py [--repeats 30] [--shapes 300:2000,1000:5000] [--its 200] [--batches 1,8,64]

The host loop of the same arithmetic (tests/cpp/two_view_host.h) on one CPU thread: tools/two_view_host_timing.cpp."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def problem(rng, n_match, n_keys, its, outliers=0.2, noise=0.1):
    """-> keys1, keys2, matches12, sets: two pinhole views (fx = fy = 500, 640 x 480) of n_match random points among n_keys keys per frame"""
    from orbhip import KP_DTYPE
    from orbhip.two_view import RAND_MAX, draw_sets
    a = np.deg2rad(4.0)
    R, t = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]), np.array([0.6, 0.05, 0.1])
    X = np.stack([rng.uniform(-2, 2, n_match), rng.uniform(-1.5, 1.5, n_match), rng.uniform(4, 8, n_match)], 1)
    X2 = X @ R.T + t
    p1 = 500 * X[:, :2] / X[:, 2:] + (320, 240) + rng.normal(0, noise, (n_match, 2))
    p2 = 500 * X2[:, :2] / X2[:, 2:] + (320, 240) + rng.normal(0, noise, (n_match, 2))
    bad = rng.random(n_match) < outliers
    p2[bad] = np.stack([rng.uniform(0, 640, bad.sum()), rng.uniform(0, 480, bad.sum())], 1)
    keys = []
    at1, at2 = np.sort(rng.choice(n_keys, n_match, replace=False)), rng.choice(n_keys, n_match, replace=False)
    for at, p in ((at1, p1), (at2, p2)):
        xy = np.stack([rng.uniform(0, 640, n_keys), rng.uniform(0, 480, n_keys)], 1)
        xy[at] = p
        k = np.zeros(n_keys, KP_DTYPE)
        k["x"], k["y"] = xy[:, 0], xy[:, 1]
        keys.append(k)
    m12 = np.full(n_keys, -1, np.int32)
    m12[at1] = at2
    return keys[0], keys[1], m12, draw_sets(n_match, its, rng.integers(0, RAND_MAX + 1, 8 * its))


def main():
    import torch
    from orbhip.two_view import TwoViewReconstruction
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--shapes", default="300:2000,1000:5000")
    ap.add_argument("--its", type=int, default=200)
    ap.add_argument("--batches", default="1,8,64")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    for shape in a.shapes.split(","):
        n_match, n_keys = [int(x) for x in shape.split(":")]
        for batch in [int(x) for x in a.batches.split(",")]:
            probs = [problem(rng, n_match, n_keys, a.its) for _ in range(batch)]
            S = TwoViewReconstruction(batch, n_keys, a.its, device="cuda:0")
            S.set_problems([p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs], [p[3] for p in probs])
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
            print(json.dumps(dict(batch=batch, matches=n_match, keys=n_keys, iterations=a.its, median_us=round(t, 1), min_us=round(min(times), 1),
                                  max_us=round(max(times), 1), per_problem_us=round(t / batch, 2), ok=int(res["ok"].sum()),
                                  model_F=int((res["model"] == 1).sum()), mean_good=float(res["n_good"].mean()))), flush=True)


if __name__ == "__main__":
    main()
