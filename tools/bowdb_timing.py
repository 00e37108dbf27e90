"""Times the place-recognition queries (orbhip.keyframe_db) on the GPU: one relocalisation query, one N-best(3) query and 64 queries in one
call against databases of 2 000 and 20 000 key frames of ~1 000 words.  Warm-up, then the median of `--repeats` event-timed calls in one
process; next to each time the bytes the dense pass must read (the word ids of every present row) divided by it.

    python tools/bowdb_timing.py [--repeats 30] [--sizes 2000,20000]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK_GBS = 8000.0   # MI355X


def world(rng, n_kf, n_words, m, cap):
    word = np.zeros((n_kf, cap), np.int32); val = np.zeros((n_kf, cap)); n = np.zeros(n_kf, np.int32)
    cur = np.unique((n_words * rng.random(m) ** 2.5).astype(np.int64))
    for i in range(n_kf):
        if i and rng.random() < 0.03:
            cur = np.unique((n_words * rng.random(m) ** 2.5).astype(np.int64))
        cur = np.unique(np.concatenate([cur[rng.random(len(cur)) < 0.85], (n_words * rng.random(m // 6) ** 2.5).astype(np.int64)]))[:cap]
        v = rng.uniform(0.5, 9.0, len(cur))
        word[i, :len(cur)] = cur; val[i, :len(cur)] = v / v.sum(); n[i] = len(cur)
    return word, val, n


def main():
    import torch
    from orbhip.keyframe_db import KeyFrameDatabase, stats_of
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--sizes", default="2000,20000")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    for n_kf in [int(x) for x in a.sizes.split(",")]:
        cap = 1280
        word, val, n = world(rng, n_kf, 1000000, 950, cap)
        db = KeyFrameDatabase(n_kf, cap, 4, "cuda:0")
        db.bv_word.copy_(torch.from_numpy(word)); db.bv_value.copy_(torch.from_numpy(val)); db.bv_n.copy_(torch.from_numpy(n))
        db.add(list(range(n_kf)), [i * 4 // n_kf for i in range(n_kf)])
        db.set_covisibles(list(range(n_kf)), [[j for j in range(i - 5, i + 6) if j != i and 0 <= j < n_kf][:10] for i in range(n_kf)])
        # queries: 64 database rows (aliasing), spread over the database
        rows = [int(r) for r in np.linspace(0, n_kf - 1, 64).astype(int)]
        q_bows = db.rows(0, n_kf)
        next_id = {"reloc": 1, "place": 1}
        dense_bytes = int(n.sum()) * 4
        for name, fam, nq in (("reloc x1", "reloc", 1), ("nbest3 x1", "place", 1), ("reloc x64", "reloc", 64), ("nbest3 x64", "place", 64)):
            Q = db.make_queries(fam, nq, cap_conn=nq)
            out, times = None, []
            for it in range(a.repeats + 5):
                ids = list(range(next_id[fam], next_id[fam] + nq)); next_id[fam] += nq
                rr = rows[:nq] if nq > 1 else [rows[(7 * it) % 64]]
                db.set_queries(Q, ids, [db.kf["map_id"][r] for r in rr], rr, conn=[[r] for r in rr] if fam == "place" else None)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = db.DetectRelocalizationCandidates(Q, q_bows, 64, out=out) if fam == "reloc" else db.DetectNBestCandidates(Q, q_bows, 3, out=out)
                e1.record()
                torch.cuda.synchronize()
                if it >= 5:
                    times.append(e0.elapsed_time(e1) * 1e3)
            st = stats_of(out)
            t = float(np.median(times)); per = t / nq
            gbs = dense_bytes / (per * 1e-6) / 1e9
            print(json.dumps(dict(case=name, key_frames=n_kf, mean_words=float(n.mean()), median_us=round(t, 1), min_us=round(min(times), 1),
                                  max_us=round(max(times), 1), per_query_us=round(per, 1), dense_mb=round(dense_bytes / 1e6, 1), gb_per_s=round(gbs, 1),
                                  hbm_fraction=round(gbs / HBM_PEAK_GBS, 4), mean_sharing=float(st["n_sharing"].mean()),
                                  mean_scored=float(st["n_scored"].mean()), max_common=int(st["max_common_words"].max()))), flush=True)


if __name__ == "__main__":
    main()
