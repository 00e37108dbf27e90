// two_view_host.h — TwoViewReconstruction::Reconstruct (reference src/TwoViewReconstruction.cc:51-1013, the Pinhole path) as a plain C++
// host loop under rule R7 of DESIGN.md section 2, operation for operation what csrc/two_view.hip and the restatement of
// tests/test_two_view.py compute.  Test infrastructure: compile with -ffp-contract=off.
#ifndef TWO_VIEW_HOST_H
#define TWO_VIEW_HOST_H
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace tvhost {

struct Result {
    bool ok = false;
    float R21[9] = {0}, t21[3] = {0}, SH = 0, SF = 0, parallax = 0;
    int bestH = -1, bestF = -1, nMatches = 0, nInliers = 0, model = -1, hypothesis = -1, nGood = 0;
    std::vector<float> p3d;          // 3 per key of frame 1
    std::vector<uint8_t> triangulated;
};

inline void gemm3(const float* A, const float* B, float* C) {   // cv::gemm of two 3x3 float matrices
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double acc = 0.0;
            for (int k = 0; k < 3; k++) acc += (double)A[i * 3 + k] * (double)B[k * 3 + j];
            C[i * 3 + j] = (float)acc;
        }
}
inline double det3(const float* S) {
    const double s00 = S[0], s01 = S[1], s02 = S[2], s10 = S[3], s11 = S[4], s12 = S[5], s20 = S[6], s21 = S[7], s22 = S[8];
    return s00 * (s11 * s22 - s12 * s21) - s01 * (s10 * s22 - s12 * s20) + s02 * (s10 * s21 - s11 * s20);
}
inline void inv3(const float* S, float* t) {   // Mat::inv()
    const double s00 = S[0], s01 = S[1], s02 = S[2], s10 = S[3], s11 = S[4], s12 = S[5], s20 = S[6], s21 = S[7], s22 = S[8];
    double d = det3(S);
    if (d != 0.0) {
        d = 1.0 / d;
        t[0] = (float)((s11 * s22 - s12 * s21) * d); t[1] = (float)((s02 * s21 - s01 * s22) * d); t[2] = (float)((s01 * s12 - s02 * s11) * d);
        t[3] = (float)((s12 * s20 - s10 * s22) * d); t[4] = (float)((s00 * s22 - s02 * s20) * d); t[5] = (float)((s02 * s10 - s00 * s12) * d);
        t[6] = (float)((s10 * s21 - s11 * s20) * d); t[7] = (float)((s01 * s20 - s00 * s21) * d); t[8] = (float)((s00 * s11 - s01 * s10) * d);
    } else {
        for (int i = 0; i < 9; i++) t[i] = 0.f;
    }
}

// the null vector of a float system A [rows][n]: cyclic Jacobi on A^T A in double, `sweeps` sweeps, the column of the least diagonal entry
inline void null_vector(const float* A, int rows, int n, int sweeps, float* v) {
    std::vector<double> M((size_t)n * n, 0.0), V((size_t)n * n, 0.0);
    for (int i = 0; i < n; i++) V[i * n + i] = 1.0;
    for (int r = 0; r < rows; r++)
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) M[i * n + j] += (double)A[r * n + i] * (double)A[r * n + j];
    for (int sweep = 0; sweep < sweeps; sweep++)
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = M[p * n + q];
                if (apq == 0.0) continue;
                const double th = (M[q * n + q] - M[p * n + p]) / (2.0 * apq);
                const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < n; k++) { const double a = M[k * n + p], b = M[k * n + q]; M[k * n + p] = c * a - sn * b; M[k * n + q] = sn * a + c * b; }
                for (int k = 0; k < n; k++) { const double a = M[p * n + k], b = M[q * n + k]; M[p * n + k] = c * a - sn * b; M[q * n + k] = sn * a + c * b; }
                for (int k = 0; k < n; k++) { const double a = V[k * n + p], b = V[k * n + q]; V[k * n + p] = c * a - sn * b; V[k * n + q] = sn * a + c * b; }
            }
    int m = 0;
    double least = M[0];
    for (int i = 1; i < n; i++) if (M[i * n + i] < least) { least = M[i * n + i]; m = i; }
    for (int k = 0; k < n; k++) v[k] = (float)V[k * n + m];
}

// svd3: one-sided Jacobi on the columns in double, 10 sweeps; w descending, U, Vt
inline void svd3(const float* A, double* w, double* U, double* Vt) {
    double G[9], V[9];
    for (int i = 0; i < 9; i++) { G[i] = (double)A[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    static const int pairs[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    for (int sweep = 0; sweep < 10; sweep++)
        for (const auto& pq : pairs) {
            const int p = pq[0], q = pq[1];
            double alpha = 0.0, beta = 0.0, gamma = 0.0;
            for (int k = 0; k < 3; k++) { alpha += G[k * 3 + p] * G[k * 3 + p]; beta += G[k * 3 + q] * G[k * 3 + q]; gamma += G[k * 3 + p] * G[k * 3 + q]; }
            if (gamma == 0.0) continue;
            const double th = (beta - alpha) / (2.0 * gamma);
            const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
            const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
            for (int k = 0; k < 3; k++) { const double a = G[k * 3 + p], b = G[k * 3 + q]; G[k * 3 + p] = c * a - sn * b; G[k * 3 + q] = sn * a + c * b; }
            for (int k = 0; k < 3; k++) { const double a = V[k * 3 + p], b = V[k * 3 + q]; V[k * 3 + p] = c * a - sn * b; V[k * 3 + q] = sn * a + c * b; }
        }
    for (int i = 0; i < 3; i++) w[i] = std::sqrt(G[i] * G[i] + G[3 + i] * G[3 + i] + G[6 + i] * G[6 + i]);
    for (int k = 0; k < 2; k++) {   // selection sort, descending, the first of equals
        int m = k;
        for (int i = k + 1; i < 3; i++) if (w[m] < w[i]) m = i;
        if (m != k) {
            std::swap(w[k], w[m]);
            for (int r = 0; r < 3; r++) { std::swap(G[r * 3 + k], G[r * 3 + m]); std::swap(V[r * 3 + k], V[r * 3 + m]); }
        }
    }
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) Vt[i * 3 + k] = V[k * 3 + i];
    if (w[0] == 0.0) { for (int i = 0; i < 9; i++) U[i] = (i % 4 == 0) ? 1.0 : 0.0; return; }
    auto cross = [&](const double* a, const double* b, int col) {
        const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
        const double n = std::sqrt(x * x + y * y + z * z);
        U[col] = x / n; U[3 + col] = y / n; U[6 + col] = z / n;
    };
    const double tiny = w[0] * 0x1p-40;
    double u0[3], u1[3];
    for (int k = 0; k < 3; k++) { u0[k] = G[k * 3] / w[0]; U[k * 3] = u0[k]; }
    if (w[1] < tiny) {
        int ax = 0;
        double least = std::fabs(u0[0]);
        if (std::fabs(u0[1]) < least) { least = std::fabs(u0[1]); ax = 1; }
        if (std::fabs(u0[2]) < least) ax = 2;
        const double e[3] = {ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0};
        cross(u0, e, 1);
    } else {
        for (int k = 0; k < 3; k++) U[k * 3 + 1] = G[k * 3 + 1] / w[1];
    }
    for (int k = 0; k < 3; k++) u1[k] = U[k * 3 + 1];
    if (w[2] < tiny) cross(u0, u1, 2);
    else for (int k = 0; k < 3; k++) U[k * 3 + 2] = G[k * 3 + 2] / w[2];
}
inline void svd3f(const float* A, float* w, float* U, float* Vt) {
    double wd[3], Ud[9], Vtd[9];
    svd3(A, wd, Ud, Vtd);
    for (int i = 0; i < 9; i++) { U[i] = (float)Ud[i]; Vt[i] = (float)Vtd[i]; }
    for (int i = 0; i < 3; i++) w[i] = (float)wd[i];
}
inline void unit3(float* t) {   // t / cv::norm(t)
    double n2 = 0.0;
    for (int i = 0; i < 3; i++) n2 += (double)t[i] * (double)t[i];
    const double alpha = 1.0 / std::sqrt(n2);
    for (int i = 0; i < 3; i++) t[i] = (float)((double)t[i] * alpha);
}

// Normalize (:833-879) over all keys
inline void normalize(const std::vector<float>& x, const std::vector<float>& y, float* mean, float* scale, float* T) {
    const int N = (int)x.size();
    float meanX = 0, meanY = 0;
    for (int i = 0; i < N; i++) { meanX += x[i]; meanY += y[i]; }
    meanX = meanX / N; meanY = meanY / N;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < N; i++) { meanDevX += std::fabs(x[i] - meanX); meanDevY += std::fabs(y[i] - meanY); }
    meanDevX = meanDevX / N; meanDevY = meanDevY / N;
    const float sX = (float)(1.0 / (double)meanDevX), sY = (float)(1.0 / (double)meanDevY);
    mean[0] = meanX; mean[1] = meanY; scale[0] = sX; scale[1] = sY;
    const float t[9] = {sX, 0.f, -meanX * sX, 0.f, sY, -meanY * sY, 0.f, 0.f, 1.f};
    std::memcpy(T, t, sizeof(t));
}

struct Motion { float R[9], t[3]; };

// CheckRT (:882-991) -> nGood; vP3D / vbGood indexed by the key of frame 1
inline int check_rt(const float* K4, const Motion& Mo, const std::vector<float>& u1, const std::vector<float>& v1, const std::vector<float>& u2,
                    const std::vector<float>& v2, const std::vector<int>& i1, const std::vector<bool>& inl, float th2, std::vector<float>& p3d,
                    std::vector<uint8_t>& good, float& parallax, bool& sawNan) {
    const float fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
    const float K[9] = {fx, 0.f, cx, 0.f, fy, cy, 0.f, 0.f, 1.f};
    const float P1[12] = {fx, 0.f, cx, 0.f, 0.f, fy, cy, 0.f, 0.f, 0.f, 1.f, 0.f};
    const float* R = Mo.R;
    const float* t = Mo.t;
    float P2[12], O2[3];
    for (int i = 0; i < 3; i++) {
        for (int c = 0; c < 4; c++) {
            double acc = 0.0;
            for (int k = 0; k < 3; k++) acc += (double)K[i * 3 + k] * (double)(c < 3 ? R[k * 3 + c] : t[k]);
            P2[i * 4 + c] = (float)acc;
        }
        double acc = 0.0;
        for (int k = 0; k < 3; k++) acc += (double)R[k * 3 + i] * (double)t[k];
        O2[i] = (float)(-1.0 * acc);
    }
    std::fill(p3d.begin(), p3d.end(), 0.f);
    std::fill(good.begin(), good.end(), 0);
    std::vector<float> vCos;
    int nGood = 0;
    sawNan = false;
    for (size_t i = 0; i < u1.size(); i++) {
        if (!inl[i]) continue;
        float A[16], v4[4], X[3];
        for (int c = 0; c < 4; c++) {
            A[c] = u1[i] * P1[8 + c] - P1[c];
            A[4 + c] = v1[i] * P1[8 + c] - P1[4 + c];
            A[8 + c] = u2[i] * P2[8 + c] - P2[c];
            A[12 + c] = v2[i] * P2[8 + c] - P2[4 + c];
        }
        null_vector(A, 4, 4, 8, v4);
        for (int k = 0; k < 3; k++) X[k] = v4[k] / v4[3];
        if (!std::isfinite(X[0]) || !std::isfinite(X[1]) || !std::isfinite(X[2])) continue;
        float n2[3];
        double q1 = 0.0, q2 = 0.0, dot = 0.0;
        for (int k = 0; k < 3; k++) { n2[k] = X[k] - O2[k]; q1 += (double)X[k] * (double)X[k]; q2 += (double)n2[k] * (double)n2[k]; dot += (double)X[k] * (double)n2[k]; }
        const float dist1 = (float)std::sqrt(q1), dist2 = (float)std::sqrt(q2);
        const float cosParallax = (float)(dot / (double)(dist1 * dist2));
        const bool low = (double)cosParallax < 0.99998;
        if (X[2] <= 0 && low) continue;
        float X2[3];
        for (int r = 0; r < 3; r++) {
            double acc = 0.0;
            for (int k = 0; k < 3; k++) acc += (double)R[r * 3 + k] * (double)X[k];
            X2[r] = (float)(acc + (double)t[r]);
        }
        if (X2[2] <= 0 && low) continue;
        const float invZ1 = (float)(1.0 / (double)X[2]);
        const float im1x = fx * X[0] * invZ1 + cx, im1y = fy * X[1] * invZ1 + cy;
        const float squareError1 = (im1x - u1[i]) * (im1x - u1[i]) + (im1y - v1[i]) * (im1y - v1[i]);
        if (squareError1 > th2) continue;
        const float invZ2 = (float)(1.0 / (double)X2[2]);
        const float im2x = fx * X2[0] * invZ2 + cx, im2y = fy * X2[1] * invZ2 + cy;
        const float squareError2 = (im2x - u2[i]) * (im2x - u2[i]) + (im2y - v2[i]) * (im2y - v2[i]);
        if (squareError2 > th2) continue;
        if (cosParallax == cosParallax) vCos.push_back(cosParallax);   // a NaN cosine is counted, not listed (R7)
        else sawNan = true;
        for (int k = 0; k < 3; k++) p3d[(size_t)i1[i] * 3 + k] = X[k];
        nGood++;
        if (low) good[i1[i]] = 1;
    }
    parallax = 0;
    if (nGood > 0 && !vCos.empty()) {
        std::sort(vCos.begin(), vCos.end());
        const size_t idx = std::min(50, int(vCos.size() - 1));
        parallax = (float)(std::acos((double)vCos[idx]) * 180.0 / 3.1415926535897932384626433832795);
    }
    return nGood;
}

// x / y of the keys of both frames, vMatches12, mvSets [its][8], K4 = fx fy cx cy
inline Result Reconstruct(const float* K4, float sigma, int its, const std::vector<float>& x1, const std::vector<float>& y1, const std::vector<float>& x2,
                          const std::vector<float>& y2, const std::vector<int>& vMatches12, const std::vector<int32_t>& sets, float minParallax = 1.0f,
                          int minTriangulated = 50) {
    Result out;
    const int n1 = (int)x1.size();
    std::vector<int> i1, i2;
    for (int i = 0; i < n1; i++)
        if (vMatches12[i] >= 0 && vMatches12[i] < (int)x2.size()) { i1.push_back(i); i2.push_back(vMatches12[i]); }
    const int N = (int)i1.size();
    out.nMatches = N;
    out.p3d.assign((size_t)n1 * 3, 0.f);
    out.triangulated.assign((size_t)n1, 0);
    if (N < 8) return out;
    float m1[2], s1[2], T1[9], m2[2], s2[2], T2[9], T2inv[9], T2t[9];
    normalize(x1, y1, m1, s1, T1);
    normalize(x2, y2, m2, s2, T2);
    inv3(T2, T2inv);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) T2t[i * 3 + j] = T2[j * 3 + i];
    std::vector<float> u1(N), v1(N), u2(N), v2(N), nu1(N), nv1(N), nu2(N), nv2(N);
    for (int i = 0; i < N; i++) {
        u1[i] = x1[i1[i]]; v1[i] = y1[i1[i]]; u2[i] = x2[i2[i]]; v2[i] = y2[i2[i]];
        nu1[i] = (u1[i] - m1[0]) * s1[0]; nv1[i] = (v1[i] - m1[1]) * s1[1]; nu2[i] = (u2[i] - m2[0]) * s2[0]; nv2[i] = (v2[i] - m2[1]) * s2[1];
    }
    const float invSigmaSquare = (float)(1.0 / (double)(sigma * sigma));
    float bestM[2][9] = {{0}, {0}};
    std::vector<bool> bestIn[2] = {std::vector<bool>(N, false), std::vector<bool>(N, false)}, cur(N);
    float S[2] = {0.f, 0.f};
    int best[2] = {-1, -1};
    for (int model = 0; model < 2; model++)
        for (int it = 0; it < its; it++) {
            const int32_t* set = &sets[(size_t)it * 8];
            float A[16 * 9], v9[9], tmp[9], M21[9], M12[9];
            for (int j = 0; j < 8; j++) {
                const float a = nu1[set[j]], b = nv1[set[j]], c = nu2[set[j]], d = nv2[set[j]];
                if (model == 0) {
                    const float r0[9] = {0.f, 0.f, 0.f, -a, -b, -1.f, d * a, d * b, d}, r1[9] = {a, b, 1.f, 0.f, 0.f, 0.f, -c * a, -c * b, -c};
                    std::memcpy(A + (2 * j) * 9, r0, sizeof(r0));
                    std::memcpy(A + (2 * j + 1) * 9, r1, sizeof(r1));
                } else {
                    const float r[9] = {c * a, c * b, c, d * a, d * b, d, a, b, 1.f};
                    std::memcpy(A + j * 9, r, sizeof(r));
                }
            }
            null_vector(A, model == 0 ? 16 : 8, 9, 12, v9);
            if (model == 0) {
                gemm3(T2inv, v9, tmp);
                gemm3(tmp, T1, M21);
                inv3(M21, M12);
            } else {
                double w[3], U[9], Vt[9];
                svd3(v9, w, U, Vt);
                float uf[9], vtf[9], D[9] = {0}, Fn[9];
                for (int i = 0; i < 9; i++) { uf[i] = (float)U[i]; vtf[i] = (float)Vt[i]; }
                D[0] = (float)w[0]; D[4] = (float)w[1];
                gemm3(uf, D, tmp);
                gemm3(tmp, vtf, Fn);
                gemm3(T2t, Fn, tmp);
                gemm3(tmp, T1, M21);
            }
            float score = 0;
            const float* m = M21;
            const float* mi = M12;
            for (int i = 0; i < N; i++) {
                bool bIn = true;
                if (model == 0) {   // CheckHomography
                    const float th = 5.991f;
                    const float w2in1inv = (float)(1.0 / (double)(mi[6] * u2[i] + mi[7] * v2[i] + mi[8]));
                    const float u2in1 = (mi[0] * u2[i] + mi[1] * v2[i] + mi[2]) * w2in1inv, v2in1 = (mi[3] * u2[i] + mi[4] * v2[i] + mi[5]) * w2in1inv;
                    const float chiSquare1 = ((u1[i] - u2in1) * (u1[i] - u2in1) + (v1[i] - v2in1) * (v1[i] - v2in1)) * invSigmaSquare;
                    if (chiSquare1 > th) bIn = false; else score += th - chiSquare1;
                    const float w1in2inv = (float)(1.0 / (double)(m[6] * u1[i] + m[7] * v1[i] + m[8]));
                    const float u1in2 = (m[0] * u1[i] + m[1] * v1[i] + m[2]) * w1in2inv, v1in2 = (m[3] * u1[i] + m[4] * v1[i] + m[5]) * w1in2inv;
                    const float chiSquare2 = ((u2[i] - u1in2) * (u2[i] - u1in2) + (v2[i] - v1in2) * (v2[i] - v1in2)) * invSigmaSquare;
                    if (chiSquare2 > th) bIn = false; else score += th - chiSquare2;
                } else {            // CheckFundamental
                    const float th = 3.841f, thScore = 5.991f;
                    const float a2 = m[0] * u1[i] + m[1] * v1[i] + m[2], b2 = m[3] * u1[i] + m[4] * v1[i] + m[5], c2 = m[6] * u1[i] + m[7] * v1[i] + m[8];
                    const float num2 = a2 * u2[i] + b2 * v2[i] + c2;
                    const float chiSquare1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * invSigmaSquare;
                    if (chiSquare1 > th) bIn = false; else score += thScore - chiSquare1;
                    const float a1 = m[0] * u2[i] + m[3] * v2[i] + m[6], b1 = m[1] * u2[i] + m[4] * v2[i] + m[7], c1 = m[2] * u2[i] + m[5] * v2[i] + m[8];
                    const float num1 = a1 * u1[i] + b1 * v1[i] + c1;
                    const float chiSquare2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * invSigmaSquare;
                    if (chiSquare2 > th) bIn = false; else score += thScore - chiSquare2;
                }
                cur[i] = bIn;
            }
            if (score > S[model]) { S[model] = score; best[model] = it; std::memcpy(bestM[model], M21, sizeof(M21)); bestIn[model] = cur; }
        }
    out.SH = S[0]; out.SF = S[1]; out.bestH = best[0]; out.bestF = best[1];
    if (S[0] + S[1] == 0.f) return out;
    const float RH = S[0] / (S[0] + S[1]);
    const int model = RH > 0.50 ? 0 : 1;
    out.model = model;
    const std::vector<bool>& inl = bestIn[model];
    int Ninl = 0;
    for (bool b : inl) Ninl += b;
    out.nInliers = Ninl;
    const float K[9] = {K4[0], 0.f, K4[2], 0.f, K4[1], K4[3], 0.f, 0.f, 1.f};
    std::vector<Motion> motions;
    float tmp[9], w[3], U[9], Vt[9];
    if (model == 1) {   // ReconstructF / DecomposeE
        const float Kt[9] = {K[0], K[3], K[6], K[1], K[4], K[7], K[2], K[5], K[8]};
        float E[9], t[3], Rr[2][9];
        gemm3(Kt, bestM[1], tmp);
        gemm3(tmp, K, E);
        svd3f(E, w, U, Vt);
        t[0] = U[2]; t[1] = U[5]; t[2] = U[8];
        unit3(t);
        const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f}, Wt[9] = {0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
        for (int k = 0; k < 2; k++) {
            gemm3(U, k ? Wt : W, tmp);
            gemm3(tmp, Vt, Rr[k]);
            if (det3(Rr[k]) < 0) for (int i = 0; i < 9; i++) Rr[k][i] = -Rr[k][i];
        }
        for (int h = 0; h < 4; h++) {
            Motion M;
            std::memcpy(M.R, Rr[h & 1], sizeof(M.R));
            for (int i = 0; i < 3; i++) M.t[i] = (h & 2) ? -t[i] : t[i];
            motions.push_back(M);
        }
    } else {            // ReconstructH
        float invK[9], A[9];
        inv3(K, invK);
        gemm3(invK, bestM[0], tmp);
        gemm3(tmp, K, A);
        svd3f(A, w, U, Vt);
        const float s = (float)(det3(U) * det3(Vt));
        const float d1 = w[0], d2 = w[1], d3 = w[2];
        if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return out;
        const float aux1 = std::sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), aux3 = std::sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
        const float x1v[4] = {aux1, aux1, -aux1, -aux1}, x3v[4] = {aux3, -aux3, aux3, -aux3};
        const float aux_stheta = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
        const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
        const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
        const float aux_sphi = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
        const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
        const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
        for (int h = 0; h < 8; h++) {
            const int i = h & 3;
            float Rp[9] = {0}, tp[3], scale;
            if (h < 4) { Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[4] = 1.f; Rp[6] = stheta[i]; Rp[8] = ctheta; tp[0] = x1v[i]; tp[1] = 0.f; tp[2] = -x3v[i]; scale = d1 - d3; }
            else { Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1.f; Rp[6] = sphi[i]; Rp[8] = -cphi; tp[0] = x1v[i]; tp[1] = 0.f; tp[2] = x3v[i]; scale = d1 + d3; }
            Motion M;
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) {
                    double acc = 0.0;
                    for (int k = 0; k < 3; k++) acc += (double)U[r * 3 + k] * (double)Rp[k * 3 + c];
                    tmp[r * 3 + c] = (float)((double)s * acc);
                }
            gemm3(tmp, Vt, M.R);
            for (int k = 0; k < 3; k++) tp[k] = (float)((double)tp[k] * (double)scale);
            for (int r = 0; r < 3; r++) {
                double acc = 0.0;
                for (int k = 0; k < 3; k++) acc += (double)U[r * 3 + k] * (double)tp[k];
                M.t[r] = (float)acc;
            }
            unit3(M.t);
            motions.push_back(M);
        }
    }
    const float th2 = (float)(4.0 * (double)(sigma * sigma));
    const int nh = (int)motions.size();
    std::vector<std::vector<float>> P(nh, std::vector<float>((size_t)n1 * 3));
    std::vector<std::vector<uint8_t>> G(nh, std::vector<uint8_t>((size_t)n1));
    std::vector<int> nGood(nh);
    std::vector<float> par(nh);
    bool nan = false;
    for (int h = 0; h < nh; h++) {
        bool sn;
        nGood[h] = check_rt(K4, motions[h], u1, v1, u2, v2, i1, inl, th2, P[h], G[h], par[h], sn);
        nan |= sn;
    }
    int win = -1;
    bool ok;
    if (model == 1) {
        const int maxGood = *std::max_element(nGood.begin(), nGood.end());
        const int nMinGood = std::max(static_cast<int>(0.9 * Ninl), minTriangulated);
        int nsimilar = 0;
        for (int h = 0; h < 4; h++) if (nGood[h] > 0.7 * maxGood) nsimilar++;
        for (int h = 3; h >= 0; h--) if (nGood[h] == maxGood) win = h;
        ok = !(maxGood < nMinGood || nsimilar > 1) && par[win] > minParallax;
        out.nGood = maxGood; out.parallax = par[win];
    } else {
        int bestGood = 0, secondBestGood = 0;
        float bestParallax = -1;
        for (int h = 0; h < 8; h++) {
            if (nGood[h] > bestGood) { secondBestGood = bestGood; bestGood = nGood[h]; win = h; bestParallax = par[h]; }
            else if (nGood[h] > secondBestGood) secondBestGood = nGood[h];
        }
        ok = secondBestGood < 0.75 * bestGood && bestParallax >= minParallax && bestGood > minTriangulated && bestGood > 0.9 * Ninl;
        out.nGood = bestGood; out.parallax = bestParallax;
    }
    if (nan) ok = false;
    out.hypothesis = win;
    out.ok = ok;
    if (ok) {
        std::memcpy(out.R21, motions[win].R, sizeof(out.R21));
        std::memcpy(out.t21, motions[win].t, sizeof(out.t21));
        out.p3d = P[win];
        out.triangulated = G[win];
    }
    return out;
}

}  // namespace tvhost
#endif
