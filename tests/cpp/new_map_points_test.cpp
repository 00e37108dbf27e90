// new_map_points_test.cpp — the adapter orbslam3_hip::NewMapPoints (search -> create for a list of neighbours on one stream, one download)
// against the path a caller has today: ORBmatcher::SearchForTriangulation through the existing adapter, the triangulation loop on the host
// (new_map_points_host.h) and the map-point flags carried by hand from one neighbour to the next.  Also: the abort predicate after neighbour 1,
// an empty neighbour list, the capacity error as an exception, a rig refused.  Built with g++ against the emulated library (CPU tier) and
// liborbhip.so (GPU tier).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include <orbslam3_hip/LocalMapping.h>
#include <orbslam3_hip/ORBmatcher.h>

#include "new_map_points_host.h"

namespace {
int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); fails++; } } while (0)

using orbslam3_hip::NewMapPoints;

struct KF {
    std::vector<orb_keypoint> kps;
    std::vector<uint8_t> desc, hasMp;
    std::vector<float> uRight, depth;
    NewMapPoints::KeyFrameView view;
    orbslam3_hip::ORBmatcher::KeyFrameView mview;
};

const float FX = 458.654f, FY = 457.296f, CX = 367.215f, CY = 248.375f, MB = 0.11f, MBF = 47.9f;

// a key frame at (ox, oy, 0) with identity rotation seeing the points X (camera-1 coordinates = world); feature order[i] = point i
void make_kf(KF& K, const std::vector<float>& X, const std::vector<uint8_t>& pointDesc, const std::vector<int>& order, float ox, float oy, bool stereo,
             int index, std::mt19937& rng) {
    const int n = (int)order.size();
    K.kps.assign(n, orb_keypoint());
    K.desc.assign((size_t)n * 32, 0);
    K.hasMp.assign(n, 0);
    K.uRight.assign(n, -1.f);
    K.depth.assign(n, -1.f);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    std::vector<std::vector<int32_t>> nodes(64);
    for (int i = 0; i < n; i++) {
        const int f = order[i];
        const float x = X[3 * i] - ox, y = X[3 * i + 1] - oy, z = X[3 * i + 2];
        std::memset(&K.kps[f], 0, sizeof(orb_keypoint));
        K.kps[f].x = FX * x / z + CX; K.kps[f].y = FY * y / z + CY; K.kps[f].octave = i % 4; K.kps[f].size = 31.f;
        std::memcpy(&K.desc[(size_t)f * 32], &pointDesc[(size_t)i * 32], 32);
        for (int b = 0; b < 3; b++) K.desc[(size_t)f * 32 + 8 + (rng() % 24)] ^= (uint8_t)(1u << (rng() % 8));   // re-observation noise, not in the node bits
        K.hasMp[f] = U(rng) < 0.2f;
        if (stereo && U(rng) < 0.5f) { K.depth[f] = z; K.uRight[f] = K.kps[f].x - MBF / z; }
    }
    for (int f = 0; f < n; f++) nodes[K.desc[(size_t)f * 32] >> 2].push_back(f);
    NewMapPoints::KeyFrameView& V = K.view;
    V.nodeId.clear(); V.nodeStart.assign(1, 0); V.featIdx.clear();
    for (int k = 0; k < 64; k++)
        if (!nodes[k].empty()) {
            V.nodeId.push_back(k);
            V.featIdx.insert(V.featIdx.end(), nodes[k].begin(), nodes[k].end());
            V.nodeStart.push_back((int32_t)V.featIdx.size());
        }
    V.N = n; V.keysUn = K.kps.data(); V.descriptors = K.desc.data(); V.hasMapPoint = K.hasMp.data();
    V.uRight = stereo ? K.uRight.data() : nullptr; V.depth = stereo ? K.depth.data() : nullptr;
    V.tcw[0] = -ox; V.tcw[1] = -oy; V.Ow[0] = ox; V.Ow[1] = oy;
    V.cameraParameters = {FX, FY, CX, CY};
    V.invfx = 1.0f / FX; V.invfy = 1.0f / FY; V.mb = MB; V.mbf = MBF;
    V.levelSigma2.clear(); V.scaleFactors.clear();
    float s = 1.f;
    for (int l = 0; l < 8; l++) { V.scaleFactors.push_back(s); V.levelSigma2.push_back(s * s); s *= 1.2f; }
    V.index = index; V.descRow0 = 1000 * index;
    K.mview.N = n; K.mview.keysUn = V.keysUn; K.mview.descriptors = V.descriptors; K.mview.uRight = V.uRight; K.mview.hasMapPoint = V.hasMapPoint;
    K.mview.nodeId = V.nodeId; K.mview.nodeStart = V.nodeStart; K.mview.featIdx = V.featIdx;
}

bool same(const NewMapPoints::Created& C, const std::vector<orbm_new_point>& ref) {
    if (C.idx1.size() != ref.size()) return false;
    for (size_t j = 0; j < ref.size(); j++)
        if (C.idx1[j] != ref[j].idx1 || C.idx2[j] != ref[j].idx2 || C.how[j] != ref[j].how || std::memcmp(&C.pos[3 * j], ref[j].pos, 12) != 0) return false;
    return true;
}
}  // namespace

int main() {
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    const int n = 300;
    std::vector<float> X(3 * n);
    std::vector<uint8_t> pointDesc((size_t)n * 32);
    for (int i = 0; i < n; i++) {
        const float z = 3.f + 5.f * U(rng);
        X[3 * i] = (U(rng) - 0.5f) * z; X[3 * i + 1] = (U(rng) - 0.5f) * 0.7f * z; X[3 * i + 2] = z;
        for (int b = 0; b < 32; b++) pointDesc[(size_t)i * 32 + b] = (uint8_t)rng();
    }
    std::vector<int> ident(n), perm(n);
    for (int i = 0; i < n; i++) ident[i] = perm[i] = i;
    KF K1;
    make_kf(K1, X, pointDesc, ident, 0.f, 0.f, true, 0, rng);
    std::vector<KF> K2(3);
    const float off[3][2] = {{0.4f, 0.05f}, {-0.5f, 0.1f}, {0.3f, -0.3f}};
    std::vector<NewMapPoints::Neighbour> nbs(3);
    for (int k = 0; k < 3; k++) {
        for (int i = n - 1; i > 0; i--) std::swap(perm[i], perm[rng() % (i + 1)]);
        make_kf(K2[k], X, pointDesc, perm, off[k][0], off[k][1], k == 1, k + 1, rng);
        nbs[k].kf = &K2[k].view;
        nbs[k].ep[0] = nbs[k].ep[1] = -1e4f;
        nbs[k].obsKf2First = k == 1;
    }

    // today's path: search (download), host loop, flags carried by hand
    std::vector<std::vector<orbm_new_point>> ref(3);
    std::vector<uint8_t> has1 = K1.hasMp;
    {
        orbslam3_hip::ORBmatcher matcher(0.6f, false);
        for (int k = 0; k < 3; k++) {
            K1.mview.hasMapPoint = has1.data();
            std::vector<std::pair<size_t, size_t>> pairs;
            matcher.SearchForTriangulation(K1.mview, K2[k].mview, nbs[k].F12, nbs[k].ep, K2[k].view.levelSigma2.data(), K2[k].view.scaleFactors.data(), 8,
                                           pairs, false, true);
            std::vector<int32_t> m12(n, -1);
            for (auto& p : pairs) m12[p.first] = (int32_t)p.second;
            const orbm_newpt_pair P = NewMapPoints::BuildPair(K1.view, K2[k].view, nbs[k].obsKf2First, false, 0.f);
            const newpt_host::Side S1{K1.kps.data(), nullptr, K1.view.uRight, K1.view.depth}, S2{K2[k].kps.data(), nullptr, K2[k].view.uRight, K2[k].view.depth};
            std::vector<uint8_t> has2 = K2[k].hasMp;
            newpt_host::create_loop(P, S1, S2, m12.data(), n, has1.data(), has2.data(), ref[k]);
            CHECK(ref[k].size() > (k == 0 ? 50u : 3u), "neighbour %d: only %zu points in the reference loop", k, ref[k].size());   // later neighbours find most features taken
        }
        K1.mview.hasMapPoint = K1.hasMp.data();
    }
    // a feature that neighbour 0 gave a point must not come back from a later neighbour
    for (int k = 1; k < 3; k++)
        for (auto& p : ref[k])
            for (auto& q : ref[0]) CHECK(p.idx1 != q.idx1, "feature %d created twice", p.idx1);

    NewMapPoints nmp;
    std::vector<NewMapPoints::Created> created;
    std::vector<uint8_t> has1After;
    int polls = 0;
    const int done = nmp.Run(K1.view, nbs, true, false, 0.f, [&] { polls++; return false; }, created, 0, &has1After);
    CHECK(done == 3 && polls == 2, "done %d polls %d", done, polls);
    for (int k = 0; k < 3; k++) CHECK(created[k].searched && same(created[k], ref[k]), "neighbour %d differs (%zu vs %zu points)", k, created[k].idx1.size(), ref[k].size());
    CHECK(has1After == has1, "hasMapPoint of the current key frame after the loop");
    CHECK(created[1].how.size() && created[0].how.size(), "points");

    // the abort predicate fires at its second poll: neighbours 0 and 1 are processed, 2 is not (LocalMapping.cc:569)
    polls = 0;
    const int done2 = nmp.Run(K1.view, nbs, true, false, 0.f, [&] { return ++polls >= 2; }, created);
    CHECK(done2 == 2 && polls == 2, "abort: done %d polls %d", done2, polls);
    CHECK(same(created[0], ref[0]) && same(created[1], ref[1]) && !created[2].searched && created[2].idx1.empty(), "abort: results");

    // an empty neighbour list
    std::vector<NewMapPoints::Neighbour> none;
    CHECK(nmp.Run(K1.view, none, true, false, 0.f, nullptr, created) == 0 && created.empty(), "empty neighbour list");

    // capacity: fewer slots than a neighbour creates
    bool threw = false;
    try { nmp.Run(K1.view, nbs, true, false, 0.f, nullptr, created, 5); } catch (const std::length_error&) { threw = true; }
    CHECK(threw, "capNew = 5 must throw std::length_error");

    // far points and a rig
    const int doneFar = nmp.Run(K1.view, nbs, true, true, 5.0f, nullptr, created);
    CHECK(doneFar == 3 && created[0].idx1.size() < ref[0].size(), "far points");
    threw = false;
    K2[1].view.hasCamera2 = true;
    try { nmp.Run(K1.view, nbs, true, false, 0.f, nullptr, created); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw, "a rig must be refused");

    if (fails == 0) std::printf("new_map_points_test OK\n");
    return fails ? 1 : 0;
}
