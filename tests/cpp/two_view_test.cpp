// two_view_test.cpp — the header-only adapter orbslam3_hip::TwoViewReconstruction against the plain C++ host loop of rule R7
// (two_view_host.h) run on the adapter's own sets: Reconstruct's return value, R21, t21, vP3D, vbTriangulated and the device's result record,
// bit for bit (with TV_GPU the parallax may differ by one float ulp: the device's acos).  Scenes: a general one, a planar one, a pure
// rotation and fewer than 8 matches (both return false with empty R21), and the overload on device pointers.  Built with g++ against the
// emulated library (CPU tier) and liborbhip.so (GPU tier).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <orbslam3_hip/TwoViewReconstruction.h>

#include "two_view_host.h"

namespace {
int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); fails++; } } while (0)

struct KeyPoint { struct { float x, y; } pt; };
struct Point3f { float x = 0, y = 0, z = 0; };

double urand(unsigned& s) { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / 16777216.0; }
double nrand(unsigned& s) { double a = 0; for (int i = 0; i < 12; i++) a += urand(s); return a - 6.0; }

struct Scene { std::vector<KeyPoint> k1, k2; std::vector<int> m12; };

// two pinhole views (fx = fy = 500, 640 x 480) of nMatch points: kind 0 general, 1 planar, 2 pure rotation; noise in pixels; every fifth match wrong;
// the matched keys interleaved with unmatched ones
Scene make_scene(int kind, int nMatch, int n1, int n2, double noise, unsigned seed) {
    Scene S;
    S.k1.resize(n1); S.k2.resize(n2); S.m12.assign(n1, -1);
    for (auto& k : S.k1) { k.pt.x = (float)(640 * urand(seed)); k.pt.y = (float)(480 * urand(seed)); }
    for (auto& k : S.k2) { k.pt.x = (float)(640 * urand(seed)); k.pt.y = (float)(480 * urand(seed)); }
    const double a = 4.0 * 3.14159265358979323846 / 180.0, t[3] = {kind == 2 ? 0.0 : 0.6, kind == 2 ? 0.0 : 0.05, kind == 2 ? 0.0 : 0.1};
    for (int j = 0; j < nMatch; j++) {
        const double x = -2 + 4 * urand(seed), y = -1.5 + 3 * urand(seed);
        const double z = kind == 1 ? 6.0 + 0.2 * x - 0.1 * y : 4 + 4 * urand(seed);
        const double x2 = std::cos(a) * x + std::sin(a) * z + t[0], y2 = y + t[1], z2 = -std::sin(a) * x + std::cos(a) * z + t[2];
        const int i1 = j * n1 / nMatch, i2 = (j * 7) % n2;   // distinct for the sizes below (7 and n2 coprime, nMatch <= n2)
        S.k1[i1].pt.x = (float)(500 * x / z + 320 + noise * nrand(seed)); S.k1[i1].pt.y = (float)(500 * y / z + 240 + noise * nrand(seed));
        if (j % 5 != 4) { S.k2[i2].pt.x = (float)(500 * x2 / z2 + 320 + noise * nrand(seed)); S.k2[i2].pt.y = (float)(500 * y2 / z2 + 240 + noise * nrand(seed)); }
        S.m12[i1] = i2;
    }
    return S;
}

bool same_parallax(float a, float b) {
#ifdef TV_GPU
    if (a != a && b != b) return true;
    int32_t ia, ib;
    std::memcpy(&ia, &a, 4); std::memcpy(&ib, &b, 4);
    return std::abs(ia - ib) <= 1 && (a < 0) == (b < 0);
#else
    return !std::memcmp(&a, &b, 4) || (a != a && b != b);
#endif
}

tvhost::Result host(const Scene& S, const std::vector<int32_t>& sets, int its) {
    const float K4[4] = {500.f, 500.f, 320.f, 240.f};
    std::vector<float> x1, y1, x2, y2;
    for (const auto& k : S.k1) { x1.push_back(k.pt.x); y1.push_back(k.pt.y); }
    for (const auto& k : S.k2) { x2.push_back(k.pt.x); y2.push_back(k.pt.y); }
    return tvhost::Reconstruct(K4, 1.0f, its, x1, y1, x2, y2, S.m12, sets);
}

void compare_record(const char* what, const orbm_tvr_result& D, const tvhost::Result& H) {
    CHECK(D.ok == (int)H.ok && D.model == H.model && D.hypothesis == H.hypothesis && D.n_good == H.nGood && D.n_inliers == H.nInliers &&
          D.n_matches == H.nMatches && D.best_it_H == H.bestH && D.best_it_F == H.bestF && !std::memcmp(&D.SH, &H.SH, 4) && !std::memcmp(&D.SF, &H.SF, 4),
          "%s: device ok %d model %d hyp %d good %d inl %d N %d best %d %d S %g %g; host ok %d model %d hyp %d good %d inl %d N %d best %d %d S %g %g", what, D.ok,
          D.model, D.hypothesis, D.n_good, D.n_inliers, D.n_matches, D.best_it_H, D.best_it_F, D.SH, D.SF, (int)H.ok, H.model, H.hypothesis, H.nGood, H.nInliers,
          H.nMatches, H.bestH, H.bestF, H.SH, H.SF);
    CHECK(same_parallax(D.parallax, H.parallax), "%s: parallax %.9g, host %.9g", what, D.parallax, H.parallax);
    CHECK(D.status == 0u, "%s: status %u", what, D.status);
}

// -> the model that won
int run(const char* what, int kind, int nMatch, int n1, int n2, double noise, int its, bool wantOk) {
    const Scene S = make_scene(kind, nMatch, n1, n2, noise, 77u + kind);
    const std::vector<float> K = {500.f, 0.f, 320.f, 0.f, 500.f, 240.f, 0.f, 0.f, 1.f};
    orbslam3_hip::TwoViewReconstruction T(K, 1.0f, its);
    std::vector<float> R21, t21;
    std::vector<Point3f> vP3D(3);   // left alone on failure
    std::vector<bool> vbTriangulated;
    const bool ok = T.Reconstruct(S.k1, S.k2, S.m12, R21, t21, vP3D, vbTriangulated);
    const tvhost::Result H = host(S, T.Sets(), its);
    compare_record(what, T.DeviceResult(), H);
    CHECK(ok == H.ok && ok == wantOk, "%s: returned %d, host loop %d, the scene was built for %d", what, ok, H.ok, wantOk);
    if (ok) {
        CHECK(R21.size() == 9 && t21.size() == 3 && !std::memcmp(R21.data(), H.R21, 36) && !std::memcmp(t21.data(), H.t21, 12), "%s: R21 / t21", what);
        CHECK((int)vP3D.size() == n1 && (int)vbTriangulated.size() == n1, "%s: %d points, %d flags", what, (int)vP3D.size(), (int)vbTriangulated.size());
        int nTri = 0;
        bool same = true;
        for (int i = 0; i < n1 && (int)vP3D.size() == n1; i++) {
            same &= !std::memcmp(&vP3D[i].x, &H.p3d[i * 3], 4) && !std::memcmp(&vP3D[i].y, &H.p3d[i * 3 + 1], 4) && !std::memcmp(&vP3D[i].z, &H.p3d[i * 3 + 2], 4);
            same &= vbTriangulated[i] == (H.triangulated[i] != 0);
            nTri += vbTriangulated[i];
        }
        CHECK(same && nTri >= 50, "%s: vP3D / vbTriangulated differ from the host loop (%d triangulated)", what, nTri);
    } else {
        CHECK(R21.empty() && t21.empty() && vP3D.size() == 3, "%s: outputs touched on failure", what);
    }
    // the overload on device pointers: its own draw of the sets, the same comparison
    std::vector<orb_keypoint> k1(n1, orb_keypoint{}), k2(n2, orb_keypoint{});
    std::vector<int32_t> m12(S.m12.begin(), S.m12.end());
    for (int i = 0; i < n1; i++) { k1[i].x = S.k1[i].pt.x; k1[i].y = S.k1[i].pt.y; }
    for (int i = 0; i < n2; i++) { k2[i].x = S.k2[i].pt.x; k2[i].y = S.k2[i].pt.y; }
    int nM = 0;
    for (int m : m12) nM += m >= 0;
    orbslam3_hip::detail::DevBuf d1, d2, dm;
    const orb_keypoint* p1 = d1.upload(k1.data(), k1.size());
    const orb_keypoint* p2 = d2.upload(k2.data(), k2.size());
    const int32_t* pm = dm.upload(m12.data(), m12.size());
    std::vector<float> R21d, t21d, P3d;
    std::vector<uint8_t> tri;
    const bool okd = T.Reconstruct(p1, n1, p2, n2, pm, nM, R21d, t21d, P3d, tri);
    const tvhost::Result Hd = host(S, T.Sets(), its);
    compare_record(what, T.DeviceResult(), Hd);
    CHECK(okd == Hd.ok, "%s (device pointers): returned %d, host loop %d", what, okd, Hd.ok);
    if (okd) CHECK(!std::memcmp(R21d.data(), Hd.R21, 36) && !std::memcmp(t21d.data(), Hd.t21, 12) && P3d.size() == Hd.p3d.size() &&
                   !std::memcmp(P3d.data(), Hd.p3d.data(), P3d.size() * 4) && tri == Hd.triangulated, "%s (device pointers): outputs", what);
    else CHECK(R21d.empty() && t21d.empty(), "%s (device pointers): R21 not empty", what);
    return H.model;
}
}  // namespace

int main() {
    const int mg = run("general", 0, 150, 200, 180, 0.2, 200, true);
    CHECK(mg == 1, "general: model %d", mg);
    run("planar", 1, 150, 200, 180, 0.2, 200, false);   // F = [e]x H fits a plane's matches for every e: no motion stands clear (or the parallax is low)
    run("rotation", 2, 150, 200, 180, 0.2, 60, false);
    {   // fewer than 8 matches: false at once, nothing drawn
        Scene S = make_scene(0, 7, 20, 20, 0.2, 5u);
        orbslam3_hip::TwoViewReconstruction T({500.f, 0.f, 320.f, 0.f, 500.f, 240.f, 0.f, 0.f, 1.f});
        std::vector<float> R21(9, 1.f), t21(3, 1.f);
        std::vector<Point3f> vP3D;
        std::vector<bool> vb;
        CHECK(!T.Reconstruct(S.k1, S.k2, S.m12, R21, t21, vP3D, vb) && R21.empty() && t21.empty() && T.DeviceResult().status == ORBM_TVR_TOO_FEW, "too few matches");
        bool threw = false;
        try { orbslam3_hip::TwoViewReconstruction bad({1.f, 2.f}); } catch (const std::invalid_argument&) { threw = true; }
        CHECK(threw, "a K of 2 floats was accepted");
    }
    if (fails) { std::printf("two_view_test: %d failure(s)\n", fails); return 1; }
    std::printf("two_view_test OK\n");
    return 0;
}
