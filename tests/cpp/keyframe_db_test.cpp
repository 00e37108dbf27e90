// keyframe_db_test.cpp — the adapter's orbslam3_hip::KeyFrameDatabase (host BowVectors in, candidate slots out, and the device-pointer
// overload) on a small hand-built database with hand-written expectations: a tie that list order decides, a merge candidate, a bad map, a
// covisible accumulated with the score an earlier query left (a stale read), erase.  The values are chosen so that every score is exact:
// query {1: .5, 2: .5} against {1: .25, 2: .25, x: .5} gives 2 * (|.25| - .5 - .25) = -1 -> 0.5, against itself 1.0 (L1Scoring::score,
// ScoringObject.cpp:23-68).  Built with g++ against the emulated library (CPU tier) and liborbhip.so (GPU tier).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <orbslam3_hip/KeyFrameDatabase.h>

namespace {
int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); fails++; } } while (0)

std::string str(const std::vector<int>& v) {
    std::string s = "[";
    for (int x : v) s += std::to_string(x) + " ";
    return s + "]";
}
}  // namespace

int main() {
    typedef std::vector<int32_t> W;
    typedef std::vector<double> V;
    orbslam3_hip::KeyFrameDatabase db(8, 8, 3);
    const W qw{1, 2};
    const V qv{0.5, 0.5};
    // slots 0, 1 (map 0), 3, 4 (map 1), 5 (map 2): score 0.5; slot 2 (map 0) equals the query: score 1.0
    const int maps[6] = {0, 0, 0, 1, 1, 2};
    for (int s = 0; s < 6; s++) {
        if (s == 2) db.add(s, maps[s], qw, qv);
        else db.add(s, maps[s], W{1, 2, 10 + s}, V{0.25, 0.25, 0.5});
    }
    db.setCovisibles(0, {1});        // acc 0.5 + 0.5 = 1.0, bestKF stays 0 (0.5 > 0.5 is false)
    db.setCovisibles(4, {3, -1, 7}); // acc 1.0; slot 7 is not present
    db.setMapBad(2, true);

    // N-best from map 0: acc = 1.0 for 0, 2, 4 (a tie: list order = add order), 0.5 for 1, 3, 5.  loop = map 0 in that order, merge = map 1;
    // slot 5 lies in the bad map
    std::vector<int> loop, merge;
    bowdb_stats st;
    db.DetectNBestCandidates(1, 0, qw, qv, {}, loop, merge, 3, &st);
    CHECK(loop == std::vector<int>({0, 2, 1}) && merge == std::vector<int>({4, 3}), "n-best: loop %s merge %s", str(loop).c_str(), str(merge).c_str());
    CHECK(st.n_sharing == 6 && st.max_common_words == 2 && st.n_scored == 6 && st.best_acc_score == 1.0f, "stats %d %d %d %g", st.n_sharing, st.max_common_words,
          st.n_scored, st.best_acc_score);
    // connected key frames are left out: without slot 0 the tie is between 2 and 4
    db.DetectNBestCandidates(2, 0, qw, qv, {0}, loop, merge, 1, &st);
    CHECK(loop == std::vector<int>({2}) && merge == std::vector<int>({4}) && st.n_sharing == 5, "connected: loop %s merge %s", str(loop).c_str(), str(merge).c_str());

    // a stale read: slot 6 equals the new query (4 common words); every other key frame shares 2 <= (int)(4 * 0.8f) = 3 and is listed but not
    // scored.  Slot 6's covisible 2 still holds the 1.0 the queries above left: acc = 1.0 + 1.0
    db.add(6, 0, W{1, 2, 3, 4}, V{0.25, 0.25, 0.25, 0.25});
    db.setCovisibles(6, {2});
    db.DetectNBestCandidates(3, 0, W{1, 2, 3, 4}, V{0.25, 0.25, 0.25, 0.25}, {}, loop, merge, 3, &st);
    CHECK(loop == std::vector<int>({6}) && merge.empty(), "stale: loop %s merge %s", str(loop).c_str(), str(merge).c_str());
    CHECK(st.n_sharing == 7 && st.max_common_words == 4 && st.n_scored == 1 && st.best_acc_score == 2.0f, "stale stats %d %d %d %g", st.n_sharing,
          st.max_common_words, st.n_scored, st.best_acc_score);

    // relocalisation (its own state family): slot 6 scores 0.5 and accumulates slot 2's 1.0 -> acc 1.5, bestKF 2; nothing else exceeds 0.75 * 1.5
    std::vector<int> cand = db.DetectRelocalizationCandidates(5, 0, qw, qv, &st);
    CHECK(cand == std::vector<int>({2}) && st.n_scored == 7 && st.best_acc_score == 1.5f, "reloc: %s %d %g", str(cand).c_str(), st.n_scored, st.best_acc_score);
    // the same from map 1: bestKF 2 lies in map 0
    cand = db.DetectRelocalizationCandidates(6, 1, qw, qv);
    CHECK(cand.empty(), "reloc other map: %s", str(cand).c_str());
    // erase slot 6: the tie of the first query is back, now in list order 0, 2, 4 for map 0
    db.erase(6);
    cand = db.DetectRelocalizationCandidates(7, 0, qw, qv, &st);
    CHECK(cand == std::vector<int>({0, 2}) && st.n_sharing == 6, "reloc after erase: %s", str(cand).c_str());
    bool refused = false;
    try { db.DetectRelocalizationCandidates(7, 0, qw, qv); } catch (const std::invalid_argument&) { refused = true; }
    CHECK(refused, "a repeated id was accepted");

    // the overload on device pointers: the caller's own query and output buffers
    {
        void *dq, *dw, *dv, *dn, *dout, *dwork;
        bool ok = orb_dev_alloc(0, sizeof(bowdb_query), &dq) == ORB_OK && orb_dev_alloc(0, 8, &dw) == ORB_OK && orb_dev_alloc(0, 16, &dv) == ORB_OK &&
                  orb_dev_alloc(0, 4, &dn) == ORB_OK && orb_dev_alloc(0, 64, &dout) == ORB_OK && orb_dev_alloc(0, bowdb_workspace_bytes(8, 1), &dwork) == ORB_OK;
        CHECK(ok, "orb_dev_alloc");
        if (ok) {
            bowdb_query q{};
            q.id = 8; q.map_id = 0;
            const int32_t n = 2;
            orb_memcpy_h2d(dq, &q, sizeof(q), nullptr); orb_memcpy_h2d(dw, qw.data(), 8, nullptr); orb_memcpy_h2d(dv, qv.data(), 16, nullptr);
            orb_memcpy_h2d(dn, &n, 4, nullptr);
            bowdb_query_bows qb{(const int32_t*)dw, (const double*)dv, (const int32_t*)dn, 1, 2};
            int32_t* o = (int32_t*)dout;
            orbslam3_hip::KeyFrameDatabase::DetectRelocalizationCandidates(db.view(), (const bowdb_query*)dq, 1, qb, o + 2, 1, o, o + 1, nullptr, dwork, nullptr);
            int32_t h[3];
            orb_memcpy_d2h(h, dout, 12, nullptr);
            orb_stream_sync(nullptr);
            CHECK(h[0] == 1 && h[1] == 2 && h[2] == 0, "device overload: n_cand %d n_required %d first %d (cap_cand 1 of 2 candidates)", h[0], h[1], h[2]);
            for (void* p : {dq, dw, dv, dn, dout, dwork}) orb_dev_free(p);
        }
    }
    if (fails) { std::printf("keyframe_db_test: %d failure(s)\n", fails); return 1; }
    std::printf("keyframe_db_test OK\n");
    return 0;
}
