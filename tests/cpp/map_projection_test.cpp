// map_projection_test.cpp — the adapter's SearchByProjectionFromMap (device projection + search) against the existing SearchByProjection
// overload fed the same map points as hand-built queries.  The hand-built queries follow integration/ORBmatcher_hip.cc's gather loops with the
// cv::Mat arithmetic of tests/cpp/mock_orbslam3 (R*X and dot products summed in double from 0, cv::norm = sqrt of the double dot,
// MapPoint::PredictScale with std::log(float)).  Built with g++ against the emulated library (CPU tier) and liborbhip.so (GPU tier).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include <orbslam3_hip/ORBmatcher.h>

namespace {
const float fx = 458.654f, fy = 457.296f, cx = 367.215f, cy = 248.375f, mbf = 47.9f, mb = 0.11f;
const int W = 752, H = 480, NL = 8;

float mat_row(const float* R, const float* X) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)R[k] * (double)X[k];
    return (float)s;
}
double dot(const float* a, const float* b) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)a[k] * (double)b[k];
    return s;
}
int predict_scale(float maxDistance, float dist, float lsf) {   // MapPoint::PredictScale, MapPoint.cc:578-610
    const float ratio = maxDistance / dist;
    int nScale = (int)std::ceil(std::log(ratio) / lsf);
    if (nScale < 0) nScale = 0; else if (nScale >= NL) nScale = NL - 1;
    return nScale;
}
float radius_by_viewing_cos(const float& viewCos) { return viewCos > 0.998 ? 2.5 : 4.0; }   // ORBmatcher.cc:260-266

int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); fails++; } } while (0)

// the queries integration/ORBmatcher_hip.cc builds for the overload `mode`, from the same records (owner[q] = map-point index)
void hand_built(int mode, const std::vector<orbm_map_point>& mps, const std::vector<uint8_t>& mpDesc, const orbm_project_frame& P,
                const orbm_project_params& prm, float lsf, std::vector<orbm_track>& track, std::vector<orbm_query>& q, std::vector<uint8_t>& qd,
                std::vector<int>& owner) {
    const float* b = P.bounds;
    int nToMatch = 0;
    for (size_t i = 0; i < mps.size(); i++) {
        const orbm_map_point& m = mps[i];
        if (!(m.flags & ORBM_MP_VALID)) continue;
        float Pc[3];
        for (int r = 0; r < 3; r++) Pc[r] = mat_row(P.Rcw + 3 * r, m.pos) + P.tcw[r];
        const float u = fx * Pc[0] / Pc[2] + cx, v = fy * Pc[1] / Pc[2] + cy;
        const bool inside = !(u < b[0] || u > b[1]) && !(v < b[2] || v > b[3]);
        float PO[3];
        for (int k = 0; k < 3; k++) PO[k] = m.pos[k] - P.Ow[k];
        const float dist = (float)std::sqrt(dot(PO, PO));
        const bool distOk = !(dist < 0.8f * m.min_distance || dist > 1.2f * m.max_distance);
        orbm_query x{};
        if (mode == ORBM_PROJ_LOCAL_MAP) {
            orbm_track& t = track[i];
            if (!(m.flags & (ORBM_MP_SEEN | ORBM_MP_BAD))) {   // Frame::isInFrustum
                t.in_view = 0; t.proj_x = -1; t.proj_y = -1;
                const float invz = 1.0f / Pc[2];
                if (!(Pc[2] < 0.0f) && inside) {
                    t.proj_x = u; t.proj_y = v;
                    if (distOk) {
                        const float viewCos = dot(PO, m.normal) / dist;
                        if (!(viewCos < prm.view_cos_limit)) {
                            t.in_view = 1; t.proj_xr = u - mbf * invz; t.depth = (float)std::sqrt(dot(Pc, Pc));
                            t.level = predict_scale(m.max_distance, dist, lsf); t.view_cos = viewCos;
                            nToMatch++;
                        }
                    }
                }
            }
            continue;   // queries after the whole list (the search runs after SearchLocalPoints' loop)
        } else if (mode == ORBM_PROJ_LAST_FRAME) {
            const float invzc = 1.0 / Pc[2];
            if (invzc < 0 || !inside) continue;
            const int o = m.octave;
            x = orbm_query{u, v, prm.th * prm.scale_factors[o], u - mbf * invzc, m.angle, (int16_t)(o - 1), (int16_t)(o + 1),
                           ORBM_Q_VALID | ((m.flags & ORBM_MP_HAS_OBS) ? ORBM_Q_HAS_OBS : 0u) | ORBM_Q_STEREO};
        } else {
            if ((m.flags & ORBM_MP_BAD) || !inside || !distOk) continue;
            const int L = predict_scale(m.max_distance, dist, lsf);
            x = orbm_query{u, v, prm.th * prm.scale_factors[L], 0.f, m.angle, (int16_t)(L - 1), (int16_t)(L + 1), ORBM_Q_VALID | ORBM_Q_HAS_OBS};
        }
        q.push_back(x); owner.push_back((int)i);
        qd.insert(qd.end(), mpDesc.begin() + (size_t)m.desc_row * 32, mpDesc.begin() + (size_t)m.desc_row * 32 + 32);
    }
    if (mode != ORBM_PROJ_LOCAL_MAP || nToMatch == 0) return;
    for (size_t i = 0; i < mps.size(); i++) {   // ORBmatcher.cc:73-110
        const orbm_map_point& m = mps[i];
        const orbm_track& t = track[i];
        if (!(m.flags & ORBM_MP_VALID) || !t.in_view || (m.flags & ORBM_MP_BAD)) continue;
        float r = radius_by_viewing_cos(t.view_cos);
        if (prm.th != 1.0) r *= prm.th;
        q.push_back(orbm_query{t.proj_x, t.proj_y, r * prm.scale_factors[t.level], t.proj_xr, 0.f, (int16_t)(t.level - 1), (int16_t)t.level,
                               ORBM_Q_VALID | ((m.flags & ORBM_MP_HAS_OBS) ? ORBM_Q_HAS_OBS : 0u) | ORBM_Q_STEREO});
        owner.push_back((int)i);
        qd.insert(qd.end(), mpDesc.begin() + (size_t)m.desc_row * 32, mpDesc.begin() + (size_t)m.desc_row * 32 + 32);
    }
}

void run_case(int mode, unsigned seed, int nmp) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    // pose: a small rotation about y and a translation; Ow = -Rcw^T tcw in the mock's arithmetic
    const float a = 0.1f, ca = std::cos(a), sa = std::sin(a);
    orbm_project_frame P{};
    const float R[9] = {ca, 0, sa, 0, 1, 0, -sa, 0, ca}, t[3] = {0.3f, -0.2f, 0.5f};
    std::memcpy(P.Rcw, R, sizeof(R)); std::memcpy(P.tcw, t, sizeof(t));
    for (int j = 0; j < 3; j++) { const float nR[3] = {-R[j], -R[3 + j], -R[6 + j]}; P.Ow[j] = mat_row(nR, t); }
    std::memcpy(P.Rlw, R, sizeof(R)); std::memcpy(P.tlw, t, sizeof(t));
    const float bnd[4] = {0.f, (float)W, 0.f, (float)H};
    std::memcpy(P.bounds, bnd, sizeof(bnd));
    float sf[NL]; sf[0] = 1.f;
    for (int l = 1; l < NL; l++) sf[l] = sf[l - 1] * 1.2f;
    const float lsf = std::log(1.2f);
    orbm_project_params prm{};
    prm.mode = mode; prm.camera_type = ORBM_CAM_PINHOLE; prm.nleft = -1; prm.fx = fx; prm.fy = fy; prm.cx = cx; prm.cy = cy; prm.mbf = mbf; prm.mb = mb;
    prm.mono = 1; prm.th = mode == ORBM_PROJ_LOCAL_MAP ? 3.f : (mode == ORBM_PROJ_LAST_FRAME ? 15.f : 10.f); prm.view_cos_limit = 0.5f;
    prm.nlevels = NL;
    for (int l = 0; l < NL; l++) prm.scale_factors[l] = sf[l];
    CHECK(orbm_predict_scale_thresholds(lsf, NL, prm.level_thresholds) == ORB_OK, "thresholds");
    // map points in front of the camera (a few behind), descriptors; the frame's keypoints near 80 % of the projections
    std::vector<orbm_map_point> mps(nmp);
    std::vector<uint8_t> mpDesc((size_t)nmp * 32);
    for (auto& c : mpDesc) c = (uint8_t)(rng() & 255);
    std::vector<orb_keypoint> kps;
    std::vector<uint8_t> kdesc;
    for (int i = 0; i < nmp; i++) {
        orbm_map_point& m = mps[i];
        const float u = -40.f + U(rng) * (W + 80), v = -40.f + U(rng) * (H + 80), z = (U(rng) < 0.08f ? -1.f : 1.f) * (0.5f + 20.f * U(rng));
        const float Xc[3] = {(u - cx) / fx * z, (v - cy) / fy * z, z};
        for (int k = 0; k < 3; k++) m.pos[k] = R[k] * (Xc[0] - t[0]) + R[3 + k] * (Xc[1] - t[1]) + R[6 + k] * (Xc[2] - t[2]);   // Rcw^T (Xc - t)
        float PO[3];
        for (int k = 0; k < 3; k++) PO[k] = m.pos[k] - P.Ow[k];
        const float d = (float)std::sqrt(dot(PO, PO));
        const float tilt = U(rng) * 1.6f;   // normal tilted from the viewing ray by up to ~92 degrees
        m.normal[0] = (PO[0] / d) * std::cos(tilt) + std::sin(tilt); m.normal[1] = PO[1] / d * std::cos(tilt); m.normal[2] = PO[2] / d * std::cos(tilt);
        const int lvl = (int)(U(rng) * NL) % NL;
        m.max_distance = d * sf[lvl] * (0.8f + 0.4f * U(rng));
        m.min_distance = m.max_distance / sf[NL - 1] * (0.8f + 0.4f * U(rng));
        m.angle = 360.f * U(rng);
        m.octave = (int)(U(rng) * NL) % NL;
        m.desc_row = i;
        m.flags = ORBM_MP_VALID | (U(rng) < 0.6f ? ORBM_MP_HAS_OBS : 0u) | (U(rng) < 0.05f ? ORBM_MP_BAD : 0u) |
                  (mode == ORBM_PROJ_LOCAL_MAP && U(rng) < 0.1f ? ORBM_MP_SEEN : 0u);
        if (U(rng) < 0.05f) m.flags = 0;
        if (z > 0 && u > 0 && u < W && v > 0 && v < H && U(rng) < 0.8f) {
            orb_keypoint k{u + (U(rng) - 0.5f) * 2.f, v + (U(rng) - 0.5f) * 2.f, 31.f, 360.f * U(rng), 1.f,
                           mode == ORBM_PROJ_LAST_FRAME ? m.octave : predict_scale(m.max_distance, d, lsf), -1};
            kps.push_back(k);
            for (int j = 0; j < 32; j++) kdesc.push_back(mpDesc[(size_t)i * 32 + j] ^ (j < 3 ? (uint8_t)(rng() & 1) : 0));
        }
    }
    std::vector<orbm_track> track0(nmp);
    for (int i = 0; i < nmp; i++) {   // stale state of an earlier frame
        track0[i] = orbm_track{U(rng) * W, U(rng) * H, U(rng) * W, 1.f + 20.f * U(rng), U(rng) < 0.5f ? 0.9985f : 0.8f, (int)(U(rng) * NL) % NL,
                               U(rng) < 0.5f ? 1 : 0, 0};
    }
    const int N = (int)kps.size();
    std::vector<uint8_t> occ(N);
    for (auto& o : occ) o = U(rng) < 0.05f ? 1 : 0;
    orbslam3_hip::FrameView F;
    F.N = N; F.keysUn = kps.data(); F.descriptors = kdesc.data(); F.occupied = occ.data();
    F.grid = orbm_grid_params{0.f, 0.f, 64.f / W, 48.f / H};
    const int thDist = mode == ORBM_PROJ_RELOC ? 64 : ORBM_TH_HIGH;
    orbslam3_hip::ORBmatcher M(mode == ORBM_PROJ_LOCAL_MAP ? 0.8f : 0.9f, true);
    // hand-built queries -> the existing overload
    std::vector<orbm_track> trackRef = track0;
    std::vector<orbm_query> q;
    std::vector<uint8_t> qd;
    std::vector<int> owner, kpRef, qMatch;
    hand_built(mode, mps, mpDesc, P, prm, lsf, trackRef, q, qd, owner);
    const int searchMode = mode == ORBM_PROJ_LOCAL_MAP ? ORBM_MODE_LOCAL_MAP : ORBM_MODE_BEST_ONLY;
    const int nRef = M.SearchByProjection(F, q, qd, searchMode, thDist, kpRef, qMatch);
    for (auto& k : kpRef) if (k >= 0) k = owner[k];
    // device projection + search
    std::vector<orbm_track> track = track0;
    std::vector<int> kpDev;
    const int nDev = M.SearchByProjectionFromMap(F, mps, mpDesc.data(), nmp, P, prm, thDist, track, kpDev);
    CHECK(nDev == nRef && nRef > 20, "mode %d: nmatches %d vs %d", mode, nDev, nRef);
    CHECK(kpDev == kpRef, "mode %d: kpMatch differs", mode);
    if (mode == ORBM_PROJ_LOCAL_MAP) CHECK(std::memcmp(track.data(), trackRef.data(), track.size() * sizeof(orbm_track)) == 0, "track states differ");
    std::printf("mode %d: %d map points, %d queries, %d keypoints, %d matches\n", mode, nmp, (int)q.size(), N, nDev);
}
}  // namespace

int main() {
    run_case(ORBM_PROJ_LOCAL_MAP, 1, 1500);
    run_case(ORBM_PROJ_LAST_FRAME, 2, 1200);
    run_case(ORBM_PROJ_RELOC, 3, 900);
    run_case(ORBM_PROJ_LOCAL_MAP, 4, 3000);   // cap_q > 2048: the search's other form
    if (fails) { std::printf("map_projection_test: %d failure(s)\n", fails); return 1; }
    std::printf("map_projection_test OK\n");
    return 0;
}
