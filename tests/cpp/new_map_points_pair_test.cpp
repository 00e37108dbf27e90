// new_map_points_pair_test.cpp — the host-only parts of orbslam3_hip::NewMapPoints (BuildCamera / BuildPair: the pair record from flattened
// key-frame views, and what they refuse) and the host loop of new_map_points_host.h on a planted scene.  Links no library: it is the program
// the sanitizer build runs (-fsanitize=address,undefined).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <orbslam3_hip/LocalMapping.h>

#include "new_map_points_host.h"

namespace {
int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); fails++; } } while (0)
using orbslam3_hip::NewMapPoints;

NewMapPoints::KeyFrameView view(float ox, int index) {
    NewMapPoints::KeyFrameView V;
    V.tcw[0] = -ox; V.Ow[0] = ox;
    V.cameraParameters = {458.654f, 457.296f, 367.215f, 248.375f};
    V.invfx = 1.0f / 458.654f; V.invfy = 1.0f / 457.296f; V.mb = 0.11f; V.mbf = 47.9f;
    float s = 1.f;
    for (int l = 0; l < 8; l++) { V.scaleFactors.push_back(s); V.levelSigma2.push_back(s * s); s *= 1.2f; }
    V.index = index; V.descRow0 = 500 * index;
    return V;
}
template <class F> bool refuses(F f) {
    try { f(); } catch (const std::invalid_argument&) { return true; }
    return false;
}
}  // namespace

int main() {
    NewMapPoints::KeyFrameView V1 = view(0.f, 3), V2 = view(0.5f, 9);
    const orbm_newpt_pair P = NewMapPoints::BuildPair(V1, V2, true, true, 20.f);
    CHECK(P.ratio_factor == 1.5f * 1.2f && P.far_points == 1 && P.th_far_points == 20.f, "pair scalars");
    CHECK(P.kf1 == 3 && P.kf2 == 9 && P.obs_kf2_first == 1 && P.desc_row0_1 == 1500 && P.desc_row0_2 == 4500, "pair indices");
    CHECK(P.cam2.tcw[0] == -0.5f && P.cam2.Ow[0] == 0.5f && P.cam2.Rcw[4] == 1.f && P.cam1.camera_type == ORBM_CAM_PINHOLE, "camera pose");
    CHECK(P.cam1.k[0] == 458.654f && P.cam1.k[4] == 0.f && P.cam1.level_sigma2[7] == V1.levelSigma2[7] && P.cam1.level_sigma2[8] == 0.f, "camera tables");
    CHECK(sizeof(orbm_newpt_pair) == 512 && sizeof(orbm_newpt_camera) == 240 && sizeof(orbm_new_point) == 24, "record sizes");
    NewMapPoints::KeyFrameView B = V2;
    B.hasCamera2 = true;
    CHECK(refuses([&] { NewMapPoints::BuildPair(V1, B, false, false, 0.f); }), "rig");
    B = V2; B.NLeft = 100;
    CHECK(refuses([&] { NewMapPoints::BuildCamera(B); }), "NLeft");
    B = V2; B.cameraType = 2;
    CHECK(refuses([&] { NewMapPoints::BuildCamera(B); }), "camera type");
    B = V2; B.cameraType = ORBM_CAM_KB8;
    CHECK(refuses([&] { NewMapPoints::BuildCamera(B); }), "KB8 with 4 parameters");
    B.cameraParameters.resize(8, 0.001f);
    CHECK(NewMapPoints::BuildCamera(B).k[7] == 0.001f, "KB8 with 8 parameters");
    B = V2; B.levelSigma2.resize(17, 1.f); B.scaleFactors.resize(17, 1.f);
    CHECK(refuses([&] { NewMapPoints::BuildCamera(B); }), "17 levels");

    // the host loop on 40 planted points 4 m away, a wrong pairing and an unmatched feature
    const int n = 40;
    std::vector<orb_keypoint> k1(n), k2(n);
    std::vector<int32_t> m12(n);
    std::vector<uint8_t> h1(n, 0), h2(n, 0);
    const orbm_newpt_pair Q = NewMapPoints::BuildPair(V1, V2, false, false, 0.f);
    for (int i = 0; i < n; i++) {
        const float x = -1.f + 0.05f * i, y = 0.3f - 0.01f * i, z = 4.f;
        std::memset(&k1[i], 0, sizeof k1[i]); std::memset(&k2[i], 0, sizeof k2[i]);
        k1[i].x = Q.cam1.k[0] * x / z + Q.cam1.k[2]; k1[i].y = Q.cam1.k[1] * y / z + Q.cam1.k[3];
        k2[i].x = Q.cam2.k[0] * (x - 0.5f) / z + Q.cam2.k[2]; k2[i].y = k1[i].y;
        k1[i].octave = k2[i].octave = i % 3;
        m12[i] = i;
    }
    m12[5] = -1;
    m12[6] = 30;
    k2[7].y += 40.f;
    const newpt_host::Side S1{k1.data(), nullptr, nullptr, nullptr}, S2{k2.data(), nullptr, nullptr, nullptr};
    std::vector<orbm_new_point> out;
    const int created = newpt_host::create_loop(Q, S1, S2, m12.data(), n, h1.data(), h2.data(), out);
    CHECK(created == n - 3 && (int)out.size() == created, "created %d", created);
    for (auto& p : out) {
        CHECK(std::fabs(p.pos[2] - 4.f) < 1e-3f && p.how == ORBM_NEWPT_CREATED_TRIANGULATED && h1[p.idx1] && h2[p.idx2], "point of feature %d: z = %f", p.idx1, p.pos[2]);
    }
    CHECK(!h1[5] && !h1[6] && !h1[7], "rejected features keep their flag");
    if (fails == 0) std::printf("new_map_points_pair_test OK\n");
    return fails ? 1 : 0;
}
