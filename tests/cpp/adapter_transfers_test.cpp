// What one steady-state call of each adapter entry point costs in runtime calls: host->device copies, memsets, device->host copies,
// synchronisations and allocations.  Pins the contract of the packed-block methods ("ONE packed host->device transfer per call ... The buffers
// only ever grow") and, for the per-array methods, the counts they have had so far.
//
// The adapters are header-only, so their orb_* calls bind to the definitions below, which count and forward to the library's own (RTLD_NEXT).
// Every entry point is called twice with the same inputs; the counts are those of the second call.  They do not depend on the sizes: a frame of
// 16 key points, 8 queries / map points, key-frame views of 16 features in 2 vocabulary nodes.
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <orbslam3_hip/Frame.h>
#include <orbslam3_hip/KeyFrameDatabase.h>
#include <orbslam3_hip/MapPoint.h>
#include <orbslam3_hip/ORBmatcher.h>

namespace {
struct Counts { int h2d, memset, d2h, sync, alloc; };
Counts g{};
template <class Fn> Fn next(const char* name) { return (Fn)dlsym(RTLD_NEXT, name); }
}  // namespace

extern "C" {
int orb_memcpy_h2d(void* d, const void* h, size_t n, void* s) {
    static auto real = next<int (*)(void*, const void*, size_t, void*)>("orb_memcpy_h2d");
    g.h2d++;
    return real(d, h, n, s);
}
int orb_memcpy_d2h(void* h, const void* d, size_t n, void* s) {
    static auto real = next<int (*)(void*, const void*, size_t, void*)>("orb_memcpy_d2h");
    g.d2h++;
    return real(h, d, n, s);
}
int orb_memset(void* d, int v, size_t n, void* s) {
    static auto real = next<int (*)(void*, int, size_t, void*)>("orb_memset");
    g.memset++;
    return real(d, v, n, s);
}
int orb_stream_sync(void* s) {
    static auto real = next<int (*)(void*)>("orb_stream_sync");
    g.sync++;
    return real(s);
}
int orb_dev_alloc(int device, size_t n, void** p) {
    static auto real = next<int (*)(int, size_t, void**)>("orb_dev_alloc");
    g.alloc++;
    return real(device, n, p);
}
int orb_host_alloc(size_t n, void** p) {
    static auto real = next<int (*)(size_t, void**)>("orb_host_alloc");
    g.alloc++;
    return real(n, p);
}
}

namespace {
int fails = 0;
// two identical calls; the second one's counts against `want`
template <class F> void expect(const char* name, const Counts& want, F call) {
    call();
    g = Counts{};
    call();
    const Counts got = g;
    std::printf("%-44s h2d %d  memset %d  d2h %d  sync %d  alloc %d\n", name, got.h2d, got.memset, got.d2h, got.sync, got.alloc);
    if (got.h2d != want.h2d || got.memset != want.memset || got.d2h != want.d2h || got.sync != want.sync || got.alloc != want.alloc) {
        std::printf("FAIL %s: expected h2d %d  memset %d  d2h %d  sync %d  alloc %d\n", name, want.h2d, want.memset, want.d2h, want.sync, want.alloc);
        fails++;
    }
}

const int N = 16, NQ = 8, W = 752, H = 480, NL = 8;
const float fx = 458.654f, fy = 457.296f, cx = 367.215f, cy = 248.375f;
uint32_t rngState = 12345u;
uint32_t rnd() { rngState = rngState * 1664525u + 1013904223u; return rngState >> 8; }
}  // namespace

int main() {
    using namespace orbslam3_hip;
    // one frame: 16 key points on a 4 x 4 lattice, random descriptors
    std::vector<orb_keypoint> kps(N);
    std::vector<uint8_t> desc((size_t)N * 32), qdesc((size_t)NQ * 32);
    std::vector<float> angle(N), uRight(N, -1.f);
    for (auto& b : desc) b = (uint8_t)rnd();
    for (int i = 0; i < N; i++) {
        kps[i] = orb_keypoint{100.f + 150.f * (i % 4), 80.f + 100.f * (i / 4), 31.f, (float)(rnd() % 360), 20.f, (int32_t)(i % 3), -1};
        angle[i] = kps[i].angle;
    }
    FrameView F;
    F.N = N; F.keysUn = kps.data(); F.descriptors = desc.data(); F.uRight = uRight.data();
    F.grid = orbm_grid_params{0.f, 0.f, 64.f / W, 48.f / H};
    // 8 queries on the first 8 key points, with their descriptors
    std::vector<orbm_query> q(NQ);
    for (int i = 0; i < NQ; i++) {
        q[i] = orbm_query{kps[i].x + 1.f, kps[i].y - 1.f, 12.f, 0.f, kps[i].angle, 0, (int16_t)(NL - 1), ORBM_Q_VALID | ORBM_Q_HAS_OBS};
        std::memcpy(&qdesc[(size_t)i * 32], &desc[(size_t)i * 32], 32);
    }
    ORBmatcher M(0.9f, true);
    std::vector<int> a, b;

    // ---- the packed-block methods: one transfer each way, nothing else (derived from the code)
    const Counts packed{1, 0, 1, 1, 0};
    expect("SearchByProjection", packed, [&] { M.SearchByProjection(F, q, qdesc, ORBM_MODE_BEST_ONLY, ORBM_TH_HIGH, a, b); });

    // 8 map points that project onto the first 8 key points from the identity pose
    std::vector<orbm_map_point> mps(NQ);
    std::vector<orbm_track> track(NQ, orbm_track{0, 0, 0, 1.f, 1.f, 0, 0, 0});
    for (int i = 0; i < NQ; i++) {
        const float z = 4.f + i;
        mps[i] = orbm_map_point{{(kps[i].x - cx) / fx * z, (kps[i].y - cy) / fy * z, z}, {0.f, 0.f, 1.f}, 0.5f * z, 2.f * z, kps[i].angle, kps[i].octave, i,
                                ORBM_MP_VALID | ORBM_MP_HAS_OBS};
    }
    orbm_project_frame pose{};
    pose.Rcw[0] = pose.Rcw[4] = pose.Rcw[8] = 1.f;
    pose.Rlw[0] = pose.Rlw[4] = pose.Rlw[8] = 1.f;
    pose.bounds[1] = (float)W; pose.bounds[3] = (float)H;
    orbm_project_params pp{};
    pp.camera_type = ORBM_CAM_PINHOLE; pp.nleft = -1; pp.fx = fx; pp.fy = fy; pp.cx = cx; pp.cy = cy; pp.mbf = 47.9f; pp.mb = 0.11f; pp.mono = 1;
    pp.view_cos_limit = 0.5f; pp.nlevels = NL;
    for (int l = 0; l < NL; l++) pp.scale_factors[l] = std::pow(1.2f, (float)l);
    if (orbm_predict_scale_thresholds(std::log(1.2f), NL, pp.level_thresholds) != ORB_OK) { std::printf("FAIL thresholds\n"); return 1; }
    pp.mode = ORBM_PROJ_LOCAL_MAP; pp.th = 3.f;
    expect("SearchByProjectionFromMap LOCAL_MAP", packed, [&] { M.SearchByProjectionFromMap(F, mps, qdesc.data(), NQ, pose, pp, ORBM_TH_HIGH, track, a); });
    pp.mode = ORBM_PROJ_LAST_FRAME; pp.th = 15.f;
    expect("SearchByProjectionFromMap LAST_FRAME", packed, [&] { M.SearchByProjectionFromMap(F, mps, qdesc.data(), NQ, pose, pp, ORBM_TH_HIGH, track, a); });

    {   // MapPointRefresh: every point seen from key frames 0 and 1, rows 2p and 2p + 1 of the key frames' descriptor slab
        MapPointRefresh R;
        std::vector<int32_t> obsStart(NQ + 1);
        std::vector<orbm_observation> obs;
        for (int p = 0; p < NQ; p++) {
            obsStart[p] = (int32_t)obs.size();
            obs.push_back(orbm_observation{0, 2 * p, 0u});
            obs.push_back(orbm_observation{1, 2 * p + 1, 0u});
        }
        obsStart[NQ] = (int32_t)obs.size();
        const std::vector<orbm_refresh_point> ref(NQ, orbm_refresh_point{0, 1});
        const std::vector<orbm_keyframe_center> kf{{{0, 0, 0}, {0.1f, 0, 0}}, {{0.5f, 0, 0}, {0.6f, 0, 0}}};
        orbm_refresh_params rp{};
        rp.what = ORBM_REFRESH_DESCRIPTOR | ORBM_REFRESH_NORMAL_DEPTH; rp.nlevels = NL;
        for (int l = 0; l < NL; l++) rp.scale_factors[l] = pp.scale_factors[l];
        std::vector<orbm_map_point> pts = mps;
        std::vector<uint8_t> mpDesc = qdesc;
        std::vector<uint32_t> status;
        const std::vector<int32_t> sel{0, 2, 5};
        expect("MapPointRefresh::Refresh", packed, [&] { R.Refresh(pts, mpDesc.data(), NQ, obsStart, obs, ref, kf, desc.data(), N, rp, a, status); });
        expect("MapPointRefresh::Refresh with sel", Counts{1, 2, 1, 1, 0},
               [&] { R.Refresh(pts, mpDesc.data(), NQ, obsStart, obs, ref, kf, desc.data(), N, rp, a, status, &sel); });
    }

    // ---- the per-array methods: the counts these calls had before the adapters shared one device-I/O helper
    expect("Fuse", Counts{6, 0, 3, 1, 0}, [&] { M.Fuse(F, q, qdesc, nullptr, NL, a, b); });
    {
        std::vector<orbm_query> q2(N);
        for (int i = 0; i < N; i++) q2[i] = orbm_query{kps[i].x, kps[i].y, 12.f, 0.f, kps[i].angle, 0, (int16_t)(NL - 1), ORBM_Q_VALID};
        expect("SearchBySim3", Counts{9, 0, 2, 3, 0}, [&] { M.SearchBySim3(F, F, q2, desc, q2, desc, a); });
    }
    std::vector<float> prev(2 * N);
    for (int i = 0; i < N; i++) { prev[2 * i] = kps[i].x; prev[2 * i + 1] = kps[i].y; }
    expect("SearchForInitialization", packed, [&] { M.SearchForInitialization(F, F, prev, a, 10); });

    // two key-frame views: 16 features in 2 vocabulary nodes
    const std::vector<uint8_t> hasMp(N, 0), hasMpAll(N, 1);
    ORBmatcher::KeyFrameView K1, K2;
    K1.N = N; K1.keysUn = kps.data(); K1.descriptors = desc.data(); K1.uRight = uRight.data(); K1.hasMapPoint = hasMp.data();
    K1.nodeId = {3, 7}; K1.nodeStart = {0, 8, 16};
    for (int i = 0; i < N; i++) K1.featIdx.push_back(i);
    K2 = K1;
    std::vector<std::pair<size_t, size_t>> pairs;
    float sigma2[16], sf[16];
    for (int l = 0; l < 16; l++) { sf[l] = std::pow(1.2f, (float)l); sigma2[l] = sf[l] * sf[l]; }
    {
        const float F12[9] = {0, -1e-6f, 2e-4f, 1e-6f, 0, -1e-3f, -2e-4f, 1e-3f, 0}, ep[2] = {-500.f, 240.f};
        expect("SearchForTriangulation", Counts{16, 0, 2, 1, 0}, [&] { M.SearchForTriangulation(K1, K2, F12, ep, sigma2, sf, NL, pairs, false); });
        orbm_tri_kb8_pair P{};
        P.n_cams = 1;
        const float k8[8] = {190.f, 190.f, 254.f, 256.f, 0.003f, 0.0007f, -0.0002f, 0.00002f};
        std::memcpy(P.k1[0], k8, sizeof(k8)); std::memcpy(P.k2[0], k8, sizeof(k8));
        P.R12[0][0] = P.R12[0][4] = P.R12[0][8] = 1.f; P.t12[0][0] = 0.2f;
        P.ep[0] = -500.f; P.ep[1] = 240.f;
        for (int l = 0; l < 16; l++) { P.level_sigma2_1[l] = P.level_sigma2_2[l] = sigma2[l]; P.scale_factors_2[l] = sf[l]; }
        expect("SearchForTriangulationKB8", Counts{14, 0, 2, 1, 0}, [&] { M.SearchForTriangulationKB8(K1, -1, K2, -1, P, pairs, false); });
    }
    K1.hasMapPoint = hasMpAll.data(); K2.hasMapPoint = hasMpAll.data();
    expect("SearchByBoW(KeyFrame, Frame)", Counts{12, 0, 2, 1, 0}, [&] { M.SearchByBoW(K1, angle.data(), K2, angle.data(), -1, a); });
    expect("SearchByBoW(KeyFrame, KeyFrame)", Counts{13, 0, 2, 1, 0}, [&] { M.SearchByBoW(K1, angle.data(), K2, angle.data(), a); });

    {
        FrameOps ops(fx, fy, cx, cy, std::vector<float>{-0.28f, 0.07f, 0.0002f, 0.00002f}, W, H);
        std::vector<orb_keypoint> un;
        expect("FrameOps::UndistortKeyPoints", Counts{2, 0, 1, 1, 0}, [&] { ops.UndistortKeyPoints(kps, un); });
    }
    {
        orbf_fisheye_rig rig{};
        const float k8[8] = {190.f, 190.f, 254.f, 256.f, 0.003f, 0.0007f, -0.0002f, 0.00002f};
        std::memcpy(rig.k_left, k8, sizeof(k8)); std::memcpy(rig.k_right, k8, sizeof(k8));
        rig.R_lr[0] = rig.R_lr[4] = rig.R_lr[8] = 1.f; rig.t_lr[0] = 0.1f;
        for (int l = 0; l < 16; l++) rig.level_sigma2[l] = sigma2[l];
        FisheyeStereoMatcher S(rig);
        std::vector<float> depth, p3d;
        expect("FisheyeStereoMatcher", Counts{5, 0, 5, 1, 0},
               [&] { S.ComputeStereoFishEyeMatches(kps, desc.data(), N / 2, kps, desc.data(), N / 2, a, b, depth, p3d); });
    }
    {
        KeyFrameDatabase db(4, 8, 1);
        const std::vector<int32_t> words{2, 5, 9};
        const std::vector<double> values{0.5, 0.3, 0.2};
        for (int slot = 0; slot < 3; slot++) db.add(slot, 0, words, values);
        uint64_t id = 0;
        expect("KeyFrameDatabase::DetectRelocalizationCandidates", Counts{4, 0, 1, 1, 0},
               [&] { db.DetectRelocalizationCandidates(++id, 0, words, values); });
    }
    if (fails) { std::printf("adapter_transfers_test: %d failure(s)\n", fails); return 1; }
    std::printf("adapter_transfers_test OK\n");
    return 0;
}
