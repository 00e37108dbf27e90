// map_refresh_test.cpp — the adapter's MapPointRefresh::Refresh (flattened host records: one packed upload, orbm_refresh_map_points, one packed
// download) against hand-built expectations: a tie the record order decides, a bad key frame, an overflow point, a selection, and the
// device-pointer overload.  The expected normals follow MapPoint::UpdateNormalAndDepth (MapPoint.cc:485-558) with the cv::Mat arithmetic of
// tests/cpp/mock_orbslam3 (cv::norm = sqrt of the double dot product, Mat / scalar = float division).  Built with g++ against the emulated
// library (CPU tier) and liborbhip.so (GPU tier).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <orbslam3_hip/MapPoint.h>

namespace {
int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); fails++; } } while (0)

const int NL = 8;
float SF[NL];

float norm3(const float* d) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)d[k] * (double)d[k];
    return (float)std::sqrt(s);
}

// a descriptor with the first `ones` bits set: the distance between two of them is |ones_a - ones_b|
void fill_desc(uint8_t* row, int ones) {
    std::memset(row, 0, 32);
    for (int b = 0; b < ones; b++) row[b >> 3] |= (uint8_t)(1u << (b & 7));
}

struct Expect { float normal[3], mn, mx; };

// MapPoint.cc:508-556 over the records [o0, o1) in order
Expect expect_normal_depth(const orbm_map_point& m, const std::vector<orbm_observation>& obs, int o0, int o1, const orbm_refresh_point& r,
                           const std::vector<orbm_keyframe_center>& kf) {
    Expect e{};
    float normal[3] = {0, 0, 0};
    int n = 0;
    for (int i = o0; i < o1; i++) {
        const float* Ow = (obs[i].flags & ORBM_OBS_RIGHT) ? kf[obs[i].kf].right : kf[obs[i].kf].left;
        float d[3];
        for (int k = 0; k < 3; k++) d[k] = m.pos[k] - Ow[k];
        const float nr = norm3(d);
        for (int k = 0; k < 3; k++) normal[k] = normal[k] + d[k] / nr;
        n++;
    }
    float PC[3];
    for (int k = 0; k < 3; k++) PC[k] = m.pos[k] - kf[r.ref_kf].left[k];
    const float dist = norm3(PC);
    e.mx = dist * SF[r.level];
    e.mn = e.mx / SF[NL - 1];
    for (int k = 0; k < 3; k++) e.normal[k] = normal[k] / (float)n;
    return e;
}
}  // namespace

int main() {
    SF[0] = 1.0f;
    for (int i = 1; i < NL; i++) SF[i] = SF[i - 1] * 1.2f;
    std::vector<orbm_keyframe_center> kf(4);
    const float centres[4][3] = {{3.f, 0.1f, 0.f}, {0.f, -0.2f, 3.f}, {-3.f, 0.05f, 0.f}, {0.f, 0.3f, -3.f}};
    for (int k = 0; k < 4; k++)
        for (int c = 0; c < 3; c++) { kf[k].left[c] = centres[k][c]; kf[k].right[c] = centres[k][c] + (c == 0 ? 0.11f : 0.f); }

    // key-frame descriptor rows: row r has `ones[r]` leading one bits
    const int ones[8] = {200, 10, 10, 40, 90, 91, 91, 0};
    const int nOver = ORBM_REFRESH_MAX_OBS + 1, nKfRows = 8 + nOver;
    std::vector<uint8_t> kfDesc((size_t)nKfRows * 32);
    for (int r = 0; r < nKfRows; r++) fill_desc(&kfDesc[(size_t)r * 32], r < 8 ? ones[r] : (r % 200));

    std::vector<orbm_observation> obs;
    std::vector<int32_t> start{0};
    // point 0, a tie: rows {200, 10, 10}: medians (lower, N = 3 -> element 1) are 190, 0, 0 -> the FIRST of the two zeros, record 1
    obs.push_back({0, 0, 0}); obs.push_back({1, 1, ORBM_OBS_RIGHT}); obs.push_back({2, 2, 0});
    start.push_back((int)obs.size());
    // point 1, a bad key frame first: usable rows {90, 91, 91} (40 is skipped) -> medians 1, 0, 0 -> record 2 (counting the skipped one);
    // with the bad record in, {40, 90, 91, 91} would give medians 50, 1, 0, 0 and the same winner, so also check N = 3's k: row 90 has median 1
    obs.push_back({3, 3, ORBM_OBS_KF_BAD}); obs.push_back({0, 4, 0}); obs.push_back({1, 5, 0}); obs.push_back({2, 6, ORBM_OBS_RIGHT});
    start.push_back((int)obs.size());
    // point 2, overflow: ORBM_REFRESH_MAX_OBS + 1 usable records
    for (int i = 0; i < nOver; i++) obs.push_back({i % 4, 8 + i, 0});
    start.push_back((int)obs.size());
    // point 3: N = 2 chooses the first; point 4: no observations
    obs.push_back({2, 7, 0}); obs.push_back({3, 0, 0});
    start.push_back((int)obs.size());
    start.push_back((int)obs.size());

    const int n = 5, nDescRows = 6;
    std::vector<orbm_map_point> mps(n);
    std::vector<orbm_refresh_point> ref(n);
    for (int p = 0; p < n; p++) {
        orbm_map_point& m = mps[p];
        std::memset(&m, 0, sizeof(m));
        m.pos[0] = 0.7f * p - 1.1f; m.pos[1] = 0.4f - 0.13f * p; m.pos[2] = 6.5f + 0.9f * p;
        m.normal[0] = 9.f; m.normal[1] = 9.f; m.normal[2] = 9.f; m.min_distance = 7.f; m.max_distance = 8.f;
        m.desc_row = (p + 2) % n; m.flags = ORBM_MP_VALID;
        ref[p].ref_kf = p % 4; ref[p].level = (p * 3) % NL;
    }
    std::vector<uint8_t> mpDesc((size_t)nDescRows * 32, 0xEE);
    orbm_refresh_params prm{};
    prm.what = ORBM_REFRESH_DESCRIPTOR | ORBM_REFRESH_NORMAL_DEPTH;
    prm.nlevels = NL;
    for (int i = 0; i < NL; i++) prm.scale_factors[i] = SF[i];

    const std::vector<orbm_map_point> mps0 = mps;
    const std::vector<uint8_t> mpDesc0 = mpDesc;
    orbslam3_hip::MapPointRefresh R;
    std::vector<int> best;
    std::vector<uint32_t> status;
    const int overflow = R.Refresh(mps, mpDesc.data(), nDescRows, start, obs, ref, kf, kfDesc.data(), nKfRows, prm, best, status);
    const uint32_t full = ORBM_REFRESHED_DESCRIPTOR | ORBM_REFRESHED_NORMAL_DEPTH;
    CHECK(overflow == 1, "overflow %d", overflow);
    CHECK(best[0] == 1 && best[1] == 2 && best[2] == -1 && best[3] == 0 && best[4] == -1, "best %d %d %d %d %d", best[0], best[1], best[2], best[3], best[4]);
    CHECK(status[0] == full && status[1] == full && status[2] == ORBM_REFRESH_OVERFLOW && status[3] == full && status[4] == 0u, "status %u %u %u %u %u",
          status[0], status[1], status[2], status[3], status[4]);
    const int winnerRow[n] = {1, 5, -1, 7, -1};
    for (int p = 0; p < n; p++) {
        const uint8_t* got = &mpDesc[(size_t)mps[p].desc_row * 32];
        if (winnerRow[p] >= 0) CHECK(!std::memcmp(got, &kfDesc[(size_t)winnerRow[p] * 32], 32), "descriptor of point %d", p);
        else CHECK(!std::memcmp(got, &mpDesc0[(size_t)mps[p].desc_row * 32], 32), "descriptor of point %d was touched", p);
        if (status[p] & ORBM_REFRESHED_NORMAL_DEPTH) {
            const Expect e = expect_normal_depth(mps0[p], obs, start[p], start[p + 1], ref[p], kf);
            CHECK(!std::memcmp(mps[p].normal, e.normal, 12) && !std::memcmp(&mps[p].min_distance, &e.mn, 4) && !std::memcmp(&mps[p].max_distance, &e.mx, 4),
                  "normal / depth of point %d: %.9g %.9g %.9g %.9g %.9g, want %.9g %.9g %.9g %.9g %.9g", p, mps[p].normal[0], mps[p].normal[1],
                  mps[p].normal[2], mps[p].min_distance, mps[p].max_distance, e.normal[0], e.normal[1], e.normal[2], e.mn, e.mx);
        } else {
            CHECK(!std::memcmp(&mps[p], &mps0[p], sizeof(orbm_map_point)), "point %d was touched", p);
        }
    }
    CHECK(!std::memcmp(&mpDesc[5 * 32], &mpDesc0[5 * 32], 32), "an unused slab row was touched");

    // a selection in non-ascending order, descriptor only: the rest is as before, the normals are not rewritten
    {
        std::vector<orbm_map_point> m2 = mps0;
        std::vector<uint8_t> d2 = mpDesc0;
        const std::vector<int32_t> sel{3, 0};
        orbm_refresh_params p2 = prm;
        p2.what = ORBM_REFRESH_DESCRIPTOR;
        const int ov = R.Refresh(m2, d2.data(), nDescRows, start, obs, ref, kf, kfDesc.data(), nKfRows, p2, best, status, &sel);
        CHECK(ov == 0 && best[0] == 1 && best[3] == 0 && best[1] == -1 && best[2] == -1 && status[1] == 0u && status[0] == ORBM_REFRESHED_DESCRIPTOR,
              "selection: %d %d %d %d", ov, best[0], best[1], best[3]);
        CHECK(!std::memcmp(m2.data(), mps0.data(), n * sizeof(orbm_map_point)), "selection: the records changed");
        CHECK(!std::memcmp(&d2[(size_t)m2[0].desc_row * 32], &kfDesc[1 * 32], 32) && !std::memcmp(&d2[(size_t)m2[1].desc_row * 32], &mpDesc0[0], 32),
              "selection: descriptors");
    }

    // the overload on device pointers: the caller's own buffers, nothing moved by the adapter
    {
        void *dmp, *dmd, *ds, *dob, *dr, *dk, *dkd, *db, *dst;
        const size_t nob = obs.size();
        bool ok = orb_dev_alloc(0, n * sizeof(orbm_map_point), &dmp) == ORB_OK && orb_dev_alloc(0, nDescRows * 32, &dmd) == ORB_OK &&
                  orb_dev_alloc(0, (n + 1) * 4, &ds) == ORB_OK && orb_dev_alloc(0, nob * sizeof(orbm_observation), &dob) == ORB_OK &&
                  orb_dev_alloc(0, n * sizeof(orbm_refresh_point), &dr) == ORB_OK && orb_dev_alloc(0, 4 * sizeof(orbm_keyframe_center), &dk) == ORB_OK &&
                  orb_dev_alloc(0, kfDesc.size(), &dkd) == ORB_OK && orb_dev_alloc(0, n * 4, &db) == ORB_OK && orb_dev_alloc(0, n * 4, &dst) == ORB_OK;
        CHECK(ok, "orb_dev_alloc");
        if (ok) {
            orb_memcpy_h2d(dmp, mps0.data(), n * sizeof(orbm_map_point), nullptr);
            orb_memcpy_h2d(dmd, mpDesc0.data(), nDescRows * 32, nullptr);
            orb_memcpy_h2d(ds, start.data(), (n + 1) * 4, nullptr);
            orb_memcpy_h2d(dob, obs.data(), nob * sizeof(orbm_observation), nullptr);
            orb_memcpy_h2d(dr, ref.data(), n * sizeof(orbm_refresh_point), nullptr);
            orb_memcpy_h2d(dk, kf.data(), 4 * sizeof(orbm_keyframe_center), nullptr);
            orb_memcpy_h2d(dkd, kfDesc.data(), kfDesc.size(), nullptr);
            orbslam3_hip::MapPointRefresh::Refresh((orbm_map_point*)dmp, n, (uint8_t*)dmd, nDescRows, nullptr, 0, (const int32_t*)ds,
                                                   (const orbm_observation*)dob, (const orbm_refresh_point*)dr, (const orbm_keyframe_center*)dk, 4,
                                                   (const uint8_t*)dkd, nKfRows, prm, (int32_t*)db, (uint32_t*)dst, nullptr);
            std::vector<orbm_map_point> m3(n);
            std::vector<uint8_t> d3((size_t)nDescRows * 32);
            std::vector<int32_t> b3(n);
            orb_memcpy_d2h(m3.data(), dmp, n * sizeof(orbm_map_point), nullptr);
            orb_memcpy_d2h(d3.data(), dmd, d3.size(), nullptr);
            orb_memcpy_d2h(b3.data(), db, n * 4, nullptr);
            orb_stream_sync(nullptr);
            CHECK(!std::memcmp(m3.data(), mps.data(), n * sizeof(orbm_map_point)) && d3 == mpDesc && b3[0] == 1 && b3[1] == 2 && b3[2] == -1,
                  "device-pointer overload differs from the host overload");
            for (void* q : {dmp, dmd, ds, dob, dr, dk, dkd, db, dst}) orb_dev_free(q);
        }
    }
    if (fails) { std::printf("map_refresh_test: %d failure(s)\n", fails); return 1; }
    std::printf("map_refresh_test OK\n");
    return 0;
}
